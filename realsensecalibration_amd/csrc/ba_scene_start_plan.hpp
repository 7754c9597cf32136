// Host-side plan of the scene start (rsba_problem_start_scene): the whole-rig start (ba_rig_start_plan.hpp) with the marker blocks as a
// third kind of block to be fitted, for a scene whose board geometry nobody measured.  Which blocks each launch of k_block_resection
// (ba_resection.hpp) fits, in which order, over which lists, with which grids and buffers.  Plain C++, header-only, from the index arrays
// alone: nothing here touches the GPU, so the unit runs under the host sanitizers (tests/scene_start_driver.cpp).
//
//   lists    the observations grouped by time, by camera and by marker (CSR: ptr[block] .. ptr[block + 1] into obs[], ascending inside a block)
//   given    the caller's flags over [C | T | M]; the base camera always; marker 0 when it is the base marker (RSBA_MODEL_MARKER_CHAIN: the
//            identity, not a block of the problem).  With every marker an ordinary block (_TEST2) marker 0 is known only if flagged.
//   rounds   a propagation from the given blocks, the kinds in turn: a TIME round fits every unknown time that has a detection whose camera
//            and marker are known, a MARKER round every unknown marker that has a detection whose camera and time are known, a CAMERA
//            round every unknown camera that has a detection whose time and marker are known.  A round that would fit nothing is not
//            launched; three empty rounds in a row end the propagation.  The plan assumes every fit succeeds; on the device a block whose
//            fit fails does not set its flag, and what only it could have reached finds no usable detection.
//   sweeps   after the rounds, refine_sweeps passes over all reached, non-given times, then markers, then cameras, each with every usable
//            detection
//   blocks no round reaches are listed as unreachable, per kind.
// Times and cameras are fitted by the whole-rig start's two kernels, which know nothing of marker flags: before such a launch
// k_scene_mask_index writes the launch's view of the detections into masked_index — the camera (time) index, or, where the detection's
// marker is not known, the index of the one flag past the C + T + M that no launch sets (SceneStartHiddenIndex).
// With every marker flagged the launches are PlanRigStart's for the same camera and time flags: a marker round is always empty, and three
// empty rounds in a row are an empty time round and an empty camera round in a row.
#pragma once
#include <climits>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "ba_rig_start_plan.hpp"

namespace rsba {

enum { kSceneStartMarker = 2 };   // RESECT_MARKER; times and cameras are kRigStartTime, kRigStartCamera

// One device allocation; offsets in bytes, every array aligned to 8.
struct SceneStartBuffers {
  size_t observations, intrinsics, distortion, parameters, own_pose, own_rms, block_rms;        // doubles
  size_t camera_index, time_index, marker_index, own_status, masked_index, time_ptr, time_obs, camera_ptr, camera_obs, marker_ptr, marker_obs,
      blocks, block_status, block_iterations;                                                  // int32
  size_t known;                                                                                  // bytes: C + T + M flags and one that is never set
  size_t total;
};

struct SceneStartPlan {
  int C = 0, T = 0, M = 0;
  int64_t N = 0;
  std::vector<int> time_ptr, time_obs, camera_ptr, camera_obs, marker_ptr, marker_obs;
  std::vector<uint8_t> given;            // [C + T + M] the flags the launches start from: the caller's, the base camera, the base marker
  std::vector<int> blocks;               // the launches' block lists, one after the other
  std::vector<RigStartLaunch> launches;  // which: kRigStartTime (a block per wavefront), kRigStartCamera, kSceneStartMarker (per workgroup)
  int num_rounds = 0;                    // launches of the propagation (the rest are sweeps)
  std::vector<int> round_of;             // [C + T + M] the round that reaches the block; -1: given; -2: unreachable
  std::vector<int> unreachable_times, unreachable_cameras, unreachable_markers;
  SceneStartBuffers buffers{};
  size_t upload_bytes = 0, download_bytes = 0;
};

// What k_scene_mask_index puts in place of a camera index (a time launch) or a time index (a camera launch, which adds C itself).
inline int32_t SceneStartHiddenIndex(int which, int C, int T, int M) { return which == kRigStartTime ? C + T + M : T + M; }

// false: an index outside its range, negative sizes, or more observations than an int indexes.  base_marker: marker 0 is the identity
// (RSBA_MODEL_MARKER_CHAIN) and always given.
inline bool PlanSceneStart(int C, int T, int M, int64_t N, const int32_t* camera_index, const int32_t* time_index, const int32_t* marker_index,
                           const uint8_t* known_blocks, bool base_marker, int refine_sweeps, bool with_distortion, SceneStartPlan* plan) {
  if (C < 0 || T < 0 || M < 0 || N < 0 || N > (int64_t)INT32_MAX || refine_sweeps < 0 || !plan) return false;
  if (N > 0 && (!camera_index || !time_index || !marker_index)) return false;
  for (int64_t i = 0; i < N; ++i)
    if (camera_index[i] < 0 || camera_index[i] >= C || time_index[i] < 0 || time_index[i] >= T || marker_index[i] < 0 || marker_index[i] >= M) return false;
  SceneStartPlan& p = *plan;
  p = SceneStartPlan();
  p.C = C; p.T = T; p.M = M; p.N = N;
  // the lists: a counting sort keeps the observation order inside a block
  auto group = [N](int n, const int32_t* key, std::vector<int>* ptr, std::vector<int>* obs) {
    ptr->assign((size_t)n + 1, 0);
    obs->assign((size_t)N, 0);
    for (int64_t i = 0; i < N; ++i) ++(*ptr)[(size_t)key[i] + 1];
    for (int b = 0; b < n; ++b) (*ptr)[(size_t)b + 1] += (*ptr)[(size_t)b];
    std::vector<int> at(ptr->begin(), ptr->end() - 1);
    for (int64_t i = 0; i < N; ++i) (*obs)[(size_t)at[(size_t)key[i]]++] = (int)i;
  };
  group(T, time_index, &p.time_ptr, &p.time_obs);
  group(C, camera_index, &p.camera_ptr, &p.camera_obs);
  group(M, marker_index, &p.marker_ptr, &p.marker_obs);

  const size_t nb = (size_t)C + T + M;
  const size_t base[3] = {(size_t)C, 0, (size_t)C + T};   // a kind's first block in [C | T | M]
  const int count_of[3] = {T, C, M};
  p.given.assign(nb, 0);
  if (known_blocks) for (size_t b = 0; b < nb; ++b) p.given[b] = known_blocks[b] ? 1 : 0;
  if (C > 0) p.given[0] = 1;                               // the base camera: the identity, not a block of the problem
  if (M > 0 && base_marker) p.given[(size_t)C + T] = 1;    // the base marker likewise
  std::vector<uint8_t> known(p.given);
  p.round_of.assign(nb, -2);
  for (size_t b = 0; b < nb; ++b) if (known[b]) p.round_of[b] = -1;

  auto lists = [&p](int which, const std::vector<int>** ptr, const std::vector<int>** obs) {
    *ptr = which == kRigStartTime ? &p.time_ptr : which == kRigStartCamera ? &p.camera_ptr : &p.marker_ptr;
    *obs = which == kRigStartTime ? &p.time_obs : which == kRigStartCamera ? &p.camera_obs : &p.marker_obs;
  };
  auto add_launch = [&p, &lists](int which, int sweep, size_t first) {
    RigStartLaunch l{};
    l.which = which;
    l.sweep = sweep;
    l.first = (int)first;
    l.count = (int)(p.blocks.size() - first);
    l.grid = RigStartGrid(which, l.count);   // a time per wavefront; a camera or a marker per workgroup
    const std::vector<int>*ptr, *obs;
    lists(which, &ptr, &obs);
    for (int k = 0; k < l.count; ++k) l.observations += (*ptr)[(size_t)p.blocks[first + (size_t)k] + 1] - (*ptr)[(size_t)p.blocks[first + (size_t)k]];
    l.list_bytes = (size_t)l.count * sizeof(int);
    l.read_bytes = (size_t)l.observations * (4 + 12 + 64);
    p.launches.push_back(l);
  };
  // a detection counts for a block of kind `which` when its two other blocks are known
  auto usable = [&](int which, int o) {
    const bool cam = known[(size_t)camera_index[o]] != 0, tim = known[(size_t)C + time_index[o]] != 0, mar = known[(size_t)C + T + marker_index[o]] != 0;
    return which == kRigStartTime ? cam && mar : which == kRigStartCamera ? tim && mar : cam && tim;
  };

  // rounds: times, markers, cameras, times, ... until three in a row add nothing
  const int turn[3] = {kRigStartTime, kSceneStartMarker, kRigStartCamera};
  int empty = 0;
  for (int round = 0; empty < 3; ++round) {
    const int which = turn[round % 3];
    const size_t first = p.blocks.size();
    const std::vector<int>*ptr, *obs;
    lists(which, &ptr, &obs);
    for (int b = 0; b < count_of[which]; ++b) {
      if (known[base[which] + (size_t)b]) continue;
      bool seen = false;
      for (int k = (*ptr)[(size_t)b]; k < (*ptr)[(size_t)b + 1] && !seen; ++k) seen = usable(which, (*obs)[(size_t)k]);
      if (seen) p.blocks.push_back(b);
    }
    if (p.blocks.size() == first) { ++empty; continue; }
    empty = 0;
    add_launch(which, 0, first);
    for (size_t k = first; k < p.blocks.size(); ++k) {
      const size_t b = base[which] + (size_t)p.blocks[k];
      known[b] = 1;
      p.round_of[b] = (int)p.launches.size() - 1;
    }
  }
  p.num_rounds = (int)p.launches.size();
  for (int t = 0; t < T; ++t) if (!known[(size_t)C + t]) p.unreachable_times.push_back(t);
  for (int c = 0; c < C; ++c) if (!known[(size_t)c]) p.unreachable_cameras.push_back(c);
  for (int m = 0; m < M; ++m) if (!known[(size_t)C + T + m]) p.unreachable_markers.push_back(m);

  // sweeps: what the rounds reached and the caller did not give
  for (int s = 1; s <= refine_sweeps; ++s) {
    for (int which : turn) {
      const size_t first = p.blocks.size();
      for (int b = 0; b < count_of[which]; ++b) if (known[base[which] + (size_t)b] && !p.given[base[which] + (size_t)b]) p.blocks.push_back(b);
      if (p.blocks.size() > first) add_launch(which, s, first);
    }
  }

  // the buffers: doubles first, then the int32 arrays, then the flags
  SceneStartBuffers& b = p.buffers;
  size_t at = 0;
  auto take = [&at](size_t bytes) { const size_t o = at; at += (bytes + 7) & ~(size_t)7; return o; };
  const size_t n = (size_t)N;
  b.observations = take(8 * n * sizeof(double));
  b.intrinsics = take(4 * (size_t)C * sizeof(double));
  b.distortion = take(with_distortion ? 5 * (size_t)C * sizeof(double) : 0);
  b.parameters = take(6 * nb * sizeof(double));
  b.own_pose = take(6 * n * sizeof(double));
  b.own_rms = take(n * sizeof(double));
  b.block_rms = take(nb * sizeof(double));
  b.camera_index = take(n * sizeof(int32_t));
  b.time_index = take(n * sizeof(int32_t));
  b.marker_index = take(n * sizeof(int32_t));
  b.own_status = take(n * sizeof(int32_t));
  b.masked_index = take(n * sizeof(int32_t));   // a time or camera launch's view of its detections: k_scene_mask_index
  b.time_ptr = take(((size_t)T + 1) * sizeof(int));
  b.time_obs = take(n * sizeof(int));
  b.camera_ptr = take(((size_t)C + 1) * sizeof(int));
  b.camera_obs = take(n * sizeof(int));
  b.marker_ptr = take(((size_t)M + 1) * sizeof(int));
  b.marker_obs = take(n * sizeof(int));
  b.blocks = take(p.blocks.size() * sizeof(int));
  b.block_status = take(nb * sizeof(int32_t));
  b.block_iterations = take(nb * sizeof(int32_t));
  b.known = take(nb + 1);
  b.total = at;
  // what crosses the bus: everything but the own fits and the masked indices goes up (the three per-block result arrays with their
  // initial values), all the blocks and the three result arrays come back
  p.upload_bytes = b.total - (b.block_rms - b.own_pose) - (b.time_ptr - b.own_status);
  p.download_bytes = 6 * nb * sizeof(double) + nb * sizeof(double) + 2 * nb * sizeof(int32_t);
  return true;
}

}  // namespace rsba
