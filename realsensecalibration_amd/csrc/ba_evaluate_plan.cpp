// Index structures of rsba_solver_evaluate's gradient kernels (ba_evaluate_plan.hpp).  Counting sorts throughout: a stable pass over
// the observations in ascending order leaves every list ascending.
#include "ba_evaluate_plan.hpp"

#include <algorithm>
#include <utility>

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

EvalMarkerIntrPlan PlanEvalMarkerIntr(int num_blocks, int C, const std::vector<EvalMarkerRow>& rows, const std::vector<uint8_t>& block_constant,
                                      const std::vector<uint8_t>& block_subset, const std::vector<int>& intr_mask) {
  EvalMarkerIntrPlan x;
  const size_t N = rows.size();
  const size_t nb = (size_t)num_blocks, nbx = nb + (size_t)C;
  const EvalMarkerLists pose = BuildEvalMarkerLists(num_blocks, rows);
  // the cameras' detections behind the pose blocks' entries: a counting sort, ascending observations
  std::vector<int> count((size_t)C, 0);
  for (const EvalMarkerRow& r : rows) count[r.camera]++;
  x.lists.ptr.assign(pose.ptr.begin(), pose.ptr.end());
  x.lists.ptr.resize(nbx + 1);
  for (int k = 0; k < C; ++k) x.lists.ptr[nb + k + 1] = x.lists.ptr[nb + k] + count[k];
  x.lists.obs = pose.obs; x.lists.slot = pose.slot;
  x.lists.obs.resize(pose.obs.size() + N); x.lists.slot.resize(pose.slot.size() + N);
  std::vector<int> fill(x.lists.ptr.begin() + nb, x.lists.ptr.end() - 1);
  for (size_t i = 0; i < N; ++i) {
    const int q = fill[rows[i].camera]++;
    x.lists.obs[q] = (int)(N + i / 3);
    x.lists.slot[q] = (unsigned char)(i % 3);
  }
  x.live = EvalMarkerLive(num_blocks, rows, block_constant);
  x.live.resize(nbx, 0);
  x.held.assign(nbx, 0);
  for (size_t b = 0; b < nb && b < block_subset.size(); ++b) x.held[b] = x.live[b] ? (unsigned char)(block_subset[b] & 63) : 0;
  for (int k = 0; k < C; ++k) {
    const int mask = (size_t)k < intr_mask.size() ? intr_mask[k] & 63 : 0;
    if (mask == 0 || count[k] == 0) continue;
    x.live[nb + k] = 1;
    x.held[nb + k] = (unsigned char)(~mask & 63);
  }
  return x;
}

static bool IsConstant(const std::vector<uint8_t>& flags, int b) { return b >= 0 && (size_t)b < flags.size() && flags[b] != 0; }

static EvalJacobianLayout FinishLayout(EvalJacobianLayout l, int rows_per_obs) {
  const size_t N = l.width.size();
  l.off.resize(N + 1);
  int64_t at = 0;
  for (size_t i = 0; i < N; ++i) { l.off[i] = at; at += (int64_t)rows_per_obs * l.width[i]; }
  l.off[N] = at;
  return l;
}

EvalJacobianLayout EvalPointJacobianLayout(int64_t N, const int32_t* camera_index, const int32_t* point_index,
                                           const std::vector<uint8_t>& camera_constant, const std::vector<uint8_t>& point_constant) {
  EvalJacobianLayout l;
  l.width.resize((size_t)N);
  for (int64_t i = 0; i < N; ++i)
    l.width[i] = (unsigned char)((IsConstant(camera_constant, camera_index[i]) ? 0 : 6) + (IsConstant(point_constant, point_index[i]) ? 0 : 3));
  return FinishLayout(std::move(l), 2);
}

EvalJacobianLayout EvalMarkerJacobianLayout(const std::vector<EvalMarkerRow>& rows, const std::vector<uint8_t>& block_constant) {
  EvalJacobianLayout l;
  l.width.resize(rows.size());
  for (size_t i = 0; i < rows.size(); ++i) {
    int w = 0;
    for (int b : {rows[i].cam_block, rows[i].time_block, rows[i].marker_block}) if (b >= 0 && !IsConstant(block_constant, b)) w += 6;
    l.width[i] = (unsigned char)w;
  }
  return FinishLayout(std::move(l), 8);
}

void EvalJacobianRowPtr(const EvalJacobianLayout& l, int rows_per_obs, int64_t* row_ptr) {
  if (!row_ptr) return;
  const size_t N = l.width.size();
  for (size_t i = 0; i < N; ++i)
    for (int r = 0; r < rows_per_obs; ++r) row_ptr[(size_t)rows_per_obs * i + r] = l.off[i] + (int64_t)r * l.width[i];
  row_ptr[(size_t)rows_per_obs * N] = l.off[N];
}

void EvalPointJacobianCols(const EvalJacobianLayout& l, int C, const int32_t* camera_index, const int32_t* point_index,
                           const std::vector<uint8_t>& camera_constant, const std::vector<uint8_t>& point_constant, int32_t* cols) {
  if (!cols) return;
  const size_t N = l.width.size();
  for (size_t i = 0; i < N; ++i) {
    const int w = l.width[i];
    int32_t* row = cols + l.off[i];
    int q = 0;
    if (!IsConstant(camera_constant, camera_index[i])) for (int a = 0; a < 6; ++a) row[q++] = 6 * camera_index[i] + a;
    if (!IsConstant(point_constant, point_index[i])) for (int a = 0; a < 3; ++a) row[q++] = 6 * C + 3 * point_index[i] + a;
    for (int a = 0; a < w; ++a) row[w + a] = row[a];
  }
}

void EvalMarkerJacobianCols(const EvalJacobianLayout& l, const std::vector<EvalMarkerRow>& rows, const std::vector<uint8_t>& block_constant,
                            int32_t* cols) {
  if (!cols) return;
  for (size_t i = 0; i < rows.size(); ++i) {
    const int w = l.width[i];
    int32_t* row = cols + l.off[i];
    int q = 0;
    for (int b : {rows[i].cam_block, rows[i].time_block, rows[i].marker_block})
      if (b >= 0 && !IsConstant(block_constant, b)) for (int a = 0; a < 6; ++a) row[q++] = 6 * b + a;
    for (int r = 1; r < 8; ++r) for (int a = 0; a < w; ++a) row[r * w + a] = row[a];
  }
}

std::vector<EvalJacobianPointRow> EvalJacobianPointRows(int P, int64_t N, const int32_t* camera_index, const int32_t* point_index,
                                                        const std::vector<int>& pt_perm) {
  std::vector<int> pos(P);
  for (int jn = 0; jn < P; ++jn) pos[pt_perm.empty() ? jn : pt_perm[jn]] = jn;
  std::vector<EvalJacobianPointRow> rows((size_t)N);
  for (int64_t i = 0; i < N; ++i) rows[i] = EvalJacobianPointRow{camera_index[i], pos[point_index[i]]};
  return rows;
}

}  // namespace rsba
