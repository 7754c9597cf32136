// Index structures of rsba_solver_evaluate's gradient kernels (ba_evaluate_plan.hpp).  Counting sorts throughout: a stable pass over
// the observations in ascending order leaves every list ascending.
#include "ba_evaluate_plan.hpp"

#include <algorithm>

namespace rsba {

std::vector<unsigned char> EvalPointLive(int C, int P, int64_t N, const int32_t* camera_index, const int32_t* point_index,
                                         const std::vector<uint8_t>& camera_constant, const std::vector<uint8_t>& point_constant) {
  std::vector<unsigned char> live((size_t)C + (size_t)P, 0);
  for (int64_t i = 0; i < N; ++i) { live[camera_index[i]] = 1; live[(size_t)C + point_index[i]] = 1; }
  const int nc = (int)std::min<size_t>(camera_constant.size(), (size_t)C), np = (int)std::min<size_t>(point_constant.size(), (size_t)P);
  for (int c = 0; c < nc; ++c) if (camera_constant[c]) live[c] = 0;
  for (int j = 0; j < np; ++j) if (point_constant[j]) live[(size_t)C + j] = 0;
  return live;
}

EvalCameraIndex BuildEvalCameraIndex(int C, int P, const std::vector<int64_t>& order, const int32_t* camera_index,
                                     const int32_t* point_index, const std::vector<int>& pt_perm) {
  EvalCameraIndex x;
  const size_t N = order.size();
  // device position of every problem point
  std::vector<int> pos(P);
  for (int jn = 0; jn < P; ++jn) pos[pt_perm.empty() ? jn : pt_perm[jn]] = jn;
  x.ptr.assign((size_t)C + 1, 0);
  for (size_t s = 0; s < N; ++s) x.ptr[(size_t)camera_index[order[s]] + 1]++;
  for (int c = 0; c < C; ++c) x.ptr[c + 1] += x.ptr[c];
  x.slot.resize(N); x.point.resize(N);
  std::vector<int> fill(x.ptr.begin(), x.ptr.end() - 1);
  for (size_t s = 0; s < N; ++s) {
    const int64_t i = order[s];
    const int q = fill[camera_index[i]]++;
    x.slot[q] = (int)s;
    x.point[q] = pos[point_index[i]];
  }
  return x;
}

EvalMarkerLists BuildEvalMarkerLists(int num_blocks, const std::vector<EvalMarkerRow>& rows) {
  EvalMarkerLists l;
  l.ptr.assign((size_t)num_blocks + 1, 0);
  auto blocks = [](const EvalMarkerRow& r, int b[3]) { b[0] = r.cam_block; b[1] = r.time_block; b[2] = r.marker_block; };
  size_t total = 0;
  for (const EvalMarkerRow& r : rows) {
    int b[3]; blocks(r, b);
    for (int k = 0; k < 3; ++k) if (b[k] >= 0) { l.ptr[(size_t)b[k] + 1]++; ++total; }
  }
  for (int b = 0; b < num_blocks; ++b) l.ptr[b + 1] += l.ptr[b];
  l.obs.resize(total); l.slot.resize(total);
  std::vector<int> fill(l.ptr.begin(), l.ptr.end() - 1);
  for (size_t i = 0; i < rows.size(); ++i) {
    int b[3]; blocks(rows[i], b);
    for (int k = 0; k < 3; ++k) {
      if (b[k] < 0) continue;
      const int q = fill[b[k]]++;
      l.obs[q] = (int)i;
      l.slot[q] = (unsigned char)k;
    }
  }
  return l;
}

std::vector<unsigned char> EvalMarkerLive(int num_blocks, const std::vector<EvalMarkerRow>& rows, const std::vector<uint8_t>& block_constant) {
  std::vector<unsigned char> live(num_blocks, 0);
  for (const EvalMarkerRow& r : rows) {
    if (r.cam_block >= 0) live[r.cam_block] = 1;
    if (r.time_block >= 0) live[r.time_block] = 1;
    if (r.marker_block >= 0) live[r.marker_block] = 1;
  }
  const int nconst = (int)std::min<size_t>(block_constant.size(), (size_t)num_blocks);
  for (int b = 0; b < nconst; ++b) if (block_constant[b]) live[b] = 0;
  return live;
}

}  // namespace rsba
