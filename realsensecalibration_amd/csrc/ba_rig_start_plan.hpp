// Host-side plan of the whole-rig start (rsba_problem_start_rig): which blocks each launch of k_block_resection (ba_resection.hpp) fits, in
// which order, over which lists, with which grids and buffers.  Plain C++, header-only, from the index arrays alone: nothing here touches
// the GPU, so the unit runs under the host sanitizers (tests/rig_start_plan_driver.cpp).
//
//   lists    the observations grouped by time and by camera (CSR: ptr[block] .. ptr[block + 1] into obs[], ascending inside a block)
//   rounds   a propagation over the co-visibility graph from the known blocks (the caller's flags; the base camera always): round 0 fits
//            every unknown time that some known camera detected, the next round every unknown camera that detected a known time, and so
//            on in turns until a round adds nothing.  The plan assumes every fit succeeds; on the device a block whose fit fails does not
//            set its flag, and what only it could have reached finds no usable detection.
//   sweeps   after the rounds, refine_sweeps passes over all reached, non-given times, then all reached, non-given cameras, each with every
//            usable detection
//   blocks no round reaches are listed as unreachable; marker blocks are inputs and always known.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace rsba {

enum { kRigStartTime = 0, kRigStartCamera = 1 };   // RESECT_TIME, RESECT_CAMERA

struct RigStartLaunch {
  int which;               // kRigStartTime: a block per wavefront, four to a workgroup; kRigStartCamera: a block per 256-lane workgroup
  int sweep;               // 0: a round of the propagation; k >= 1: the k-th refining sweep
  int first, count;        // its blocks: blocks[first .. first + count)
  unsigned grid;           // workgroups of 256 lanes
  int64_t observations;    // detections on its blocks' lists
  size_t list_bytes;       // bytes of its block list
  size_t read_bytes;       // per pass over its lists: index of the list (4), three block indices (12), eight corner values (64) a detection
};

// One device allocation; offsets in bytes, every array aligned to 8.
struct RigStartBuffers {
  size_t observations, intrinsics, distortion, parameters, own_pose, own_rms, block_rms;        // doubles
  size_t camera_index, time_index, marker_index, own_status, time_ptr, time_obs, camera_ptr, camera_obs, blocks, block_status,
      block_iterations;                                                                        // int32
  size_t known;                                                                                  // bytes
  size_t total;
};

struct RigStartPlan {
  int C = 0, T = 0, M = 0;
  int64_t N = 0;
  std::vector<int> time_ptr, time_obs, camera_ptr, camera_obs;
  std::vector<uint8_t> given;            // [C + T] the flags the launches start from: the caller's, and the base camera
  std::vector<int> blocks;               // the launches' block lists, one after the other
  std::vector<RigStartLaunch> launches;
  int num_rounds = 0;                    // launches of the propagation (the rest are sweeps)
  std::vector<int> round_of;             // [C + T] the round that reaches the block; -1: given; -2: unreachable
  std::vector<int> unreachable_times, unreachable_cameras;
  RigStartBuffers buffers{};
  size_t upload_bytes = 0, download_bytes = 0;
};

inline unsigned RigStartGrid(int which, int count) { return which == kRigStartTime ? (unsigned)((count + 3) / 4) : (unsigned)count; }

// false: an index outside its range, negative sizes, or more observations than an int indexes.
inline bool PlanRigStart(int C, int T, int M, int64_t N, const int32_t* camera_index, const int32_t* time_index, const uint8_t* known_blocks,
                         int refine_sweeps, bool with_distortion, RigStartPlan* plan) {
  if (C < 0 || T < 0 || M < 0 || N < 0 || N > (int64_t)INT32_MAX || refine_sweeps < 0 || !plan) return false;
  if (N > 0 && (!camera_index || !time_index)) return false;
  for (int64_t i = 0; i < N; ++i)
    if (camera_index[i] < 0 || camera_index[i] >= C || time_index[i] < 0 || time_index[i] >= T) return false;
  RigStartPlan& p = *plan;
  p = RigStartPlan();
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

  p.given.assign((size_t)C + T, 0);
  if (known_blocks) for (int b = 0; b < C + T; ++b) p.given[(size_t)b] = known_blocks[b] ? 1 : 0;
  if (C > 0) p.given[0] = 1;   // the base camera: the identity, not a block of the problem
  std::vector<uint8_t> known(p.given);
  p.round_of.assign((size_t)C + T, -2);
  for (int b = 0; b < C + T; ++b) if (known[(size_t)b]) p.round_of[(size_t)b] = -1;

  auto add_launch = [&p](int which, int sweep, size_t first) {
    RigStartLaunch l{};
    l.which = which;
    l.sweep = sweep;
    l.first = (int)first;
    l.count = (int)(p.blocks.size() - first);
    l.grid = RigStartGrid(which, l.count);
    const std::vector<int>& ptr = which == kRigStartTime ? p.time_ptr : p.camera_ptr;
    for (int k = 0; k < l.count; ++k) l.observations += ptr[(size_t)p.blocks[first + (size_t)k] + 1] - ptr[(size_t)p.blocks[first + (size_t)k]];
    l.list_bytes = (size_t)l.count * sizeof(int);
    l.read_bytes = (size_t)l.observations * (4 + 12 + 64);
    p.launches.push_back(l);
  };

  // rounds: times, cameras, times, ... until one adds nothing (an empty time round still lets the camera round try once: with every camera
  // given and no unknown time the first round is empty and so is the second)
  int empty = 0;
  for (int round = 0; empty < 2; ++round) {
    const int which = round % 2 == 0 ? kRigStartTime : kRigStartCamera;
    const size_t first = p.blocks.size();
    if (which == kRigStartTime) {
      for (int t = 0; t < T; ++t) {
        if (known[(size_t)C + t]) continue;
        bool seen = false;
        for (int k = p.time_ptr[(size_t)t]; k < p.time_ptr[(size_t)t + 1] && !seen; ++k) seen = known[(size_t)camera_index[p.time_obs[(size_t)k]]] != 0;
        if (seen) p.blocks.push_back(t);
      }
    } else {
      for (int c = 0; c < C; ++c) {
        if (known[(size_t)c]) continue;
        bool seen = false;
        for (int k = p.camera_ptr[(size_t)c]; k < p.camera_ptr[(size_t)c + 1] && !seen; ++k) seen = known[(size_t)C + time_index[p.camera_obs[(size_t)k]]] != 0;
        if (seen) p.blocks.push_back(c);
      }
    }
    if (p.blocks.size() == first) { ++empty; continue; }
    empty = 0;
    add_launch(which, 0, first);
    for (size_t k = first; k < p.blocks.size(); ++k) {
      const size_t b = which == kRigStartTime ? (size_t)C + p.blocks[k] : (size_t)p.blocks[k];
      known[b] = 1;
      p.round_of[b] = (int)p.launches.size() - 1;
    }
  }
  p.num_rounds = (int)p.launches.size();
  for (int t = 0; t < T; ++t) if (!known[(size_t)C + t]) p.unreachable_times.push_back(t);
  for (int c = 0; c < C; ++c) if (!known[(size_t)c]) p.unreachable_cameras.push_back(c);

  // sweeps: what the rounds reached and the caller did not give
  for (int s = 1; s <= refine_sweeps; ++s) {
    size_t first = p.blocks.size();
    for (int t = 0; t < T; ++t) if (known[(size_t)C + t] && !p.given[(size_t)C + t]) p.blocks.push_back(t);
    if (p.blocks.size() > first) add_launch(kRigStartTime, s, first);
    first = p.blocks.size();
    for (int c = 0; c < C; ++c) if (known[(size_t)c] && !p.given[(size_t)c]) p.blocks.push_back(c);
    if (p.blocks.size() > first) add_launch(kRigStartCamera, s, first);
  }

  // the buffers: doubles first, then the int32 arrays, then the flags
  RigStartBuffers& b = p.buffers;
  size_t at = 0;
  auto take = [&at](size_t bytes) { const size_t o = at; at += (bytes + 7) & ~(size_t)7; return o; };
  const size_t n = (size_t)N, nb = (size_t)C + T;
  b.observations = take(8 * n * sizeof(double));
  b.intrinsics = take(4 * (size_t)C * sizeof(double));
  b.distortion = take(with_distortion ? 5 * (size_t)C * sizeof(double) : 0);
  b.parameters = take(6 * (nb + (size_t)M) * sizeof(double));
  b.own_pose = take(6 * n * sizeof(double));
  b.own_rms = take(n * sizeof(double));
  b.block_rms = take(nb * sizeof(double));
  b.camera_index = take(n * sizeof(int32_t));
  b.time_index = take(n * sizeof(int32_t));
  b.marker_index = take(n * sizeof(int32_t));
  b.own_status = take(n * sizeof(int32_t));
  b.time_ptr = take(((size_t)T + 1) * sizeof(int));
  b.time_obs = take(n * sizeof(int));
  b.camera_ptr = take(((size_t)C + 1) * sizeof(int));
  b.camera_obs = take(n * sizeof(int));
  b.blocks = take(p.blocks.size() * sizeof(int));
  b.block_status = take(nb * sizeof(int32_t));
  b.block_iterations = take(nb * sizeof(int32_t));
  b.known = take(nb);
  b.total = at;
  // what crosses the bus: everything but the own fits goes up (the three per-block result arrays with their initial values), the
  // camera and time blocks and the three result arrays come back
  p.upload_bytes = b.total - (b.block_rms - b.own_pose) - (b.time_ptr - b.own_status);
  p.download_bytes = 6 * nb * sizeof(double) + nb * sizeof(double) + 2 * nb * sizeof(int32_t);
  return true;
}

}  // namespace rsba
