// C ABI: problem container, options, file formats (no device code here).  Declared in include/rsba.h.
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "ba_problem.hpp"
#include "ba_solver.hpp"

extern "C" {

int rsba_version(void) { return RSBA_VERSION; }
int rsba_device_count(void) { return rsba::DeviceCount(); }

const char* rsba_error_string(int code) {
  switch (code) {
    case RSBA_OK: return "ok";
    case RSBA_ERR_IO: return "unable to open file";
    case RSBA_ERR_FORMAT: return "malformed file";
    case RSBA_ERR_ARG: return "bad argument";
    case RSBA_ERR_HIP: return "HIP runtime error";
    case RSBA_ERR_NO_DEVICE: return "no HIP device (this library has no CPU path)";
    case RSBA_ERR_COMM: return "RCCL error";
    case RSBA_ERR_UNSUPPORTED: return "unsupported configuration";
    case RSBA_ERR_RANK_DEFICIENT: return "rank deficient: the covariance does not exist";
    default: return "unknown error";
  }
}

int rsba_problem_create_points(int32_t C, int32_t P, int64_t N, const int32_t* camera_index, const int32_t* point_index,
                               const double* observations, const double* parameters, const double* intrinsics, rsba_problem** out) {
  if (C <= 0 || P <= 0 || N < 0 || !camera_index || !point_index || !observations || !parameters || !intrinsics || !out) return RSBA_ERR_ARG;
  for (int64_t i = 0; i < N; ++i)
    if (camera_index[i] < 0 || camera_index[i] >= C || point_index[i] < 0 || point_index[i] >= P) return RSBA_ERR_ARG;
  rsba_problem* p = new rsba_problem();
  p->model = RSBA_MODEL_POINTS; p->num_cameras = C; p->num_points = P; p->num_observations = N;
  p->camera_index.assign(camera_index, camera_index + N);
  p->point_index.assign(point_index, point_index + N);
  p->observations.assign(observations, observations + 2 * N);
  p->parameters.assign(parameters, parameters + 6 * (size_t)C + 3 * (size_t)P);
  p->intrinsics.assign(intrinsics, intrinsics + 4 * (size_t)C);
  *out = p;
  return RSBA_OK;
}

int rsba_problem_create_marker_chain(int32_t model, int32_t C, int32_t T, int32_t M, int64_t N, const int32_t* time_index,
                                     const int32_t* camera_index, const int32_t* marker_index, const double* observations,
                                     const double* parameters, const double* intrinsics, double marker_side, rsba_problem** out) {
  if ((model != RSBA_MODEL_MARKER_CHAIN && model != RSBA_MODEL_MARKER_CHAIN_TEST2) || C <= 0 || T <= 0 || M <= 0 || N < 0 || N > INT32_MAX ||
      !time_index || !camera_index || !marker_index || !observations || !parameters || !intrinsics || !(marker_side > 0.0) || !out)
    return RSBA_ERR_ARG;
  for (int64_t i = 0; i < N; ++i)
    if (time_index[i] < 0 || time_index[i] >= T || camera_index[i] < 0 || camera_index[i] >= C || marker_index[i] < 0 || marker_index[i] >= M)
      return RSBA_ERR_ARG;
  rsba_problem* p = new rsba_problem();
  p->model = model; p->num_cameras = C; p->num_times = T; p->num_markers = M; p->num_observations = N; p->marker_side = marker_side;
  p->time_index.assign(time_index, time_index + N);
  p->camera_index.assign(camera_index, camera_index + N);
  p->marker_index.assign(marker_index, marker_index + N);
  p->observations.assign(observations, observations + 8 * N);
  p->parameters.assign(parameters, parameters + 6 * ((size_t)C + T + M));
  p->intrinsics.assign(intrinsics, intrinsics + 4 * (size_t)C);
  p->obs_per_time_camera.assign((size_t)T * C, 0);
  for (int64_t i = 0; i < N; ++i) p->obs_per_time_camera[(size_t)time_index[i] * C + camera_index[i]]++;
  *out = p;
  return RSBA_OK;
}

int rsba_problem_load_points_file(const char* path, const double* intrinsics4, rsba_problem** out) { return rsba::LoadPointsFile(path, intrinsics4, out); }
int rsba_problem_load_correspondence(const char* path, int32_t model, double marker_side, const double* intrinsics, rsba_problem** out) {
  return rsba::LoadCorrespondence(path, model, marker_side, intrinsics, out);
}
int rsba_problem_set_camera_constant(rsba_problem* p, int32_t camera_idx, int32_t constant) {
  if (!p || camera_idx < 0 || camera_idx >= p->num_cameras) return RSBA_ERR_ARG;
  if (p->model != RSBA_MODEL_POINTS) return RSBA_ERR_UNSUPPORTED;   // the marker-chain wiring already fixes camera 0 / marker 0
  if (p->camera_constant.empty()) p->camera_constant.assign(p->num_cameras, 0);
  p->camera_constant[camera_idx] = constant ? 1 : 0;
  return RSBA_OK;
}
int rsba_problem_set_point_constant(rsba_problem* p, int32_t point_idx, int32_t constant) {
  if (!p || point_idx < 0 || point_idx >= p->num_points) return RSBA_ERR_ARG;
  if (p->model != RSBA_MODEL_POINTS) return RSBA_ERR_UNSUPPORTED;
  if (p->point_constant.empty()) p->point_constant.assign(p->num_points, 0);
  p->point_constant[point_idx] = constant ? 1 : 0;
  return RSBA_OK;
}
int rsba_problem_set_parameter_block_constant(rsba_problem* p, int64_t parameter_offset, int32_t constant) {
  if (!p || parameter_offset < 0 || parameter_offset >= (int64_t)p->parameters.size()) return RSBA_ERR_ARG;
  if (p->model == RSBA_MODEL_POINTS) {
    const int64_t cam_end = 6LL * p->num_cameras;
    if (parameter_offset < cam_end) return parameter_offset % 6 ? RSBA_ERR_ARG : rsba_problem_set_camera_constant(p, (int32_t)(parameter_offset / 6), constant);
    return (parameter_offset - cam_end) % 3 ? RSBA_ERR_ARG : rsba_problem_set_point_constant(p, (int32_t)((parameter_offset - cam_end) / 3), constant);
  }
  if (parameter_offset % 6) return RSBA_ERR_ARG;
  const size_t nblocks = (size_t)p->num_cameras + p->num_times + p->num_markers;
  if (p->block_constant.empty()) p->block_constant.assign(nblocks, 0);
  p->block_constant[(size_t)(parameter_offset / 6)] = constant ? 1 : 0;
  return RSBA_OK;
}
int rsba_problem_set_parameter_subset_constant(rsba_problem* p, int64_t parameter_offset, int32_t constant_mask) {
  if (!p) return RSBA_ERR_ARG;
  if (!p->is_marker_chain()) return RSBA_ERR_UNSUPPORTED;   // the point model's camera rows sit in the headline kernels
  const int64_t nblocks = (int64_t)p->num_cameras + p->num_times + p->num_markers;
  if (parameter_offset < 0 || parameter_offset >= 6 * nblocks || parameter_offset % 6) return RSBA_ERR_ARG;
  if (constant_mask < 0 || constant_mask >= 63) return RSBA_ERR_ARG;   // all six: the block call (Ceres 1.14 CHECK-fails)
  if (p->block_subset.empty()) p->block_subset.assign((size_t)nblocks, 0);
  p->block_subset[(size_t)(parameter_offset / 6)] = (uint8_t)constant_mask;
  return RSBA_OK;
}
int32_t rsba_problem_parameter_subset_constant(const rsba_problem* p, int64_t parameter_offset) {
  if (!p || !p->is_marker_chain() || parameter_offset < 0 || parameter_offset % 6) return 0;
  return parameter_offset / 6 < (int64_t)p->block_subset.size() ? p->block_subset[(size_t)(parameter_offset / 6)] : 0;
}
int rsba_problem_set_observation_weights(rsba_problem* p, const double* weights) {
  if (!p) return RSBA_ERR_ARG;
  if (!p->is_marker_chain()) return RSBA_ERR_UNSUPPORTED;   // the point model's loss sites take no per-observation factor
  if (!weights) { p->observation_weights.clear(); return RSBA_OK; }
  for (int64_t i = 0; i < p->num_observations; ++i) if (!std::isfinite(weights[i]) || weights[i] < 0.0) return RSBA_ERR_ARG;
  p->observation_weights.assign(weights, weights + p->num_observations);
  return RSBA_OK;
}
const double* rsba_problem_observation_weights(const rsba_problem* p) {
  return (p && !p->observation_weights.empty()) ? p->observation_weights.data() : nullptr;
}
int rsba_problem_set_distortion(rsba_problem* p, const double* dist) {
  if (!p) return RSBA_ERR_ARG;
  if (!p->is_marker_chain()) return RSBA_ERR_UNSUPPORTED;   // the point model's projection sits in the headline kernels
  if (!dist) { p->distortion.clear(); return RSBA_OK; }
  const size_t n = 5 * (size_t)p->num_cameras;
  for (size_t i = 0; i < n; ++i) if (!std::isfinite(dist[i])) return RSBA_ERR_ARG;
  p->distortion.assign(dist, dist + n);
  return RSBA_OK;
}
const double* rsba_problem_distortion(const rsba_problem* p) {
  return (p && !p->distortion.empty()) ? p->distortion.data() : nullptr;
}
int rsba_problem_set_intrinsics_free(rsba_problem* p, int32_t camera_idx, int32_t free_mask) {
  if (!p) return RSBA_ERR_ARG;
  if (!p->is_marker_chain()) return RSBA_ERR_UNSUPPORTED;   // like distortion: the point model's projection sits in the headline kernels
  if (camera_idx < 0 || camera_idx >= p->num_cameras || free_mask < 0 || free_mask > 63) return RSBA_ERR_ARG;
  if (p->intrinsics_free.empty()) p->intrinsics_free.assign((size_t)p->num_cameras, 0);
  p->intrinsics_free[(size_t)camera_idx] = (uint8_t)free_mask;
  return RSBA_OK;
}
int32_t rsba_problem_intrinsics_free(const rsba_problem* p, int32_t camera_idx) {
  return (p && p->is_marker_chain()) ? p->intrinsics_free_mask(camera_idx) : 0;
}
const double* rsba_problem_intrinsics(const rsba_problem* p) { return p ? p->intrinsics.data() : nullptr; }
// the block a prior may sit on: a camera or marker block that is a parameter block of the model's wiring (-1 - code otherwise)
static int PriorBlock(const rsba_problem* p, int64_t parameter_offset) {
  if (!p) return -1 - RSBA_ERR_ARG;
  if (!p->is_marker_chain()) return -1 - RSBA_ERR_UNSUPPORTED;   // like weights, distortion and subsets
  const int64_t C = p->num_cameras, T = p->num_times, M = p->num_markers;
  if (parameter_offset < 0 || parameter_offset >= 6 * (C + T + M) || parameter_offset % 6) return -1 - RSBA_ERR_ARG;
  const int64_t b = parameter_offset / 6;
  if (b >= C && b < C + T) return -1 - RSBA_ERR_UNSUPPORTED;     // time blocks are the eliminated ones
  // the wiring's fixed base blocks are no parameter blocks
  if (b == 0 || (b == C + T && p->model == RSBA_MODEL_MARKER_CHAIN)) return -1 - RSBA_ERR_ARG;
  return (int)b;
}
int rsba_problem_set_block_prior(rsba_problem* p, int64_t parameter_offset, const double* A, const double* b) {
  const int blk = PriorBlock(p, parameter_offset);
  if (blk < 0) return -1 - blk;
  if (!A) { p->block_priors.erase(blk); return RSBA_OK; }
  if (!b) return RSBA_ERR_ARG;
  for (int i = 0; i < 36; ++i) if (!std::isfinite(A[i])) return RSBA_ERR_ARG;
  for (int i = 0; i < 6; ++i) if (!std::isfinite(b[i])) return RSBA_ERR_ARG;
  std::array<double, 42>& v = p->block_priors[blk];
  std::copy(A, A + 36, v.begin());
  std::copy(b, b + 6, v.begin() + 36);
  return RSBA_OK;
}
int rsba_problem_block_prior(const rsba_problem* p, int64_t parameter_offset, double* A, double* b) {
  if (!p || !p->is_marker_chain() || parameter_offset < 0 || parameter_offset % 6) return 0;
  if (parameter_offset >= 6 * ((int64_t)p->num_cameras + p->num_times + p->num_markers)) return 0;
  const auto it = p->block_priors.find((int)(parameter_offset / 6));
  if (it == p->block_priors.end()) return 0;
  if (A) std::copy(it->second.begin(), it->second.begin() + 36, A);
  if (b) std::copy(it->second.begin() + 36, it->second.end(), b);
  return 1;
}
int32_t rsba_problem_num_block_priors(const rsba_problem* p) { return p ? (int32_t)p->block_priors.size() : 0; }
void rsba_problem_free(rsba_problem* p) { delete p; }

int rsba_base_pose_from_marker_detection(const double* marker_from_camera, const double* marker_from_base, double* base_from_camera) {
  if (!marker_from_camera || !marker_from_base || !base_from_camera) return RSBA_ERR_ARG;
  rsba::BaseFromMarkerDetection(marker_from_camera, marker_from_base, base_from_camera);
  return RSBA_OK;
}
int rsba_marker_pose_in_camera(const double* base_from_camera, const double* marker_from_base, double* marker_from_camera) {
  if (!base_from_camera || !marker_from_base || !marker_from_camera) return RSBA_ERR_ARG;
  rsba::MarkerFromCamera(base_from_camera, marker_from_base, marker_from_camera);
  return RSBA_OK;
}
int rsba_marker_corners_in_camera(const double* pose, double marker_side, double* out12) {
  if (!pose || !out12 || !(marker_side > 0.0)) return RSBA_ERR_ARG;
  rsba::MarkerCornersInCamera(pose, marker_side, out12);
  return RSBA_OK;
}
int rsba_solve_pnp_epnp(int32_t n, const double* object_points, const double* image_points, const double* intrinsics4, double* pose) {
  return rsba::SolvePnPEPnP(n, object_points, image_points, intrinsics4, pose);
}
int rsba_problem_initial_camera_poses(rsba_problem* p) { return rsba::InitialCameraPoses(p); }
int rsba_marker_pose_from_corners(const double* corners8, const double* intrinsics4, const double* dist5_or_null, double marker_side,
                                  double* pose6, double* rms_or_null, int32_t* status_or_null) {
  return rsba::MarkerPoseFromCorners(corners8, intrinsics4, dist5_or_null, marker_side, pose6, rms_or_null, status_or_null);
}
int rsba_marker_pose_from_corners_both(const double* corners8, const double* intrinsics4, const double* dist5_or_null, double marker_side,
                                       double* poses12, double* rms2_or_null, int32_t* status2_or_null) {
  return rsba::MarkerPoseFromCornersBoth(corners8, intrinsics4, dist5_or_null, marker_side, poses12, rms2_or_null, status2_or_null);
}
int rsba_problem_initial_time_poses(rsba_problem* p, int32_t* num_missing_or_null) { return rsba::InitialTimePoses(p, num_missing_or_null); }

int32_t rsba_problem_model(const rsba_problem* p) { return p ? p->model : -1; }
int32_t rsba_problem_num_cameras(const rsba_problem* p) { return p ? p->num_cameras : 0; }
int32_t rsba_problem_num_points(const rsba_problem* p) { return p ? p->num_points : 0; }
int32_t rsba_problem_num_times(const rsba_problem* p) { return p ? p->num_times : 0; }
int32_t rsba_problem_num_markers(const rsba_problem* p) { return p ? p->num_markers : 0; }
int64_t rsba_problem_num_observations(const rsba_problem* p) { return p ? p->num_observations : 0; }
int64_t rsba_problem_num_parameters(const rsba_problem* p) { return p ? p->num_parameters() : 0; }
int32_t rsba_problem_num_observations_per_time_camera(const rsba_problem* p, int32_t t, int32_t c) {
  if (!p || !p->is_marker_chain() || t < 0 || t >= p->num_times || c < 0 || c >= p->num_cameras) return 0;
  return p->obs_per_time_camera[t * p->num_cameras + c] * 4;  // bundle_adjustment.cpp:29-32
}
const double* rsba_problem_observations(const rsba_problem* p) { return p ? p->observations.data() : nullptr; }
double* rsba_problem_parameters(rsba_problem* p) { return p ? p->parameters.data() : nullptr; }
int32_t rsba_problem_camera_idx(const rsba_problem* p, int64_t i) { return (p && i >= 0 && i < p->num_observations) ? p->camera_index[i] : -1; }
int32_t rsba_problem_point_idx(const rsba_problem* p, int64_t i) { return (p && !p->is_marker_chain() && i >= 0 && i < p->num_observations) ? p->point_index[i] : -1; }
int32_t rsba_problem_time_idx(const rsba_problem* p, int64_t i) { return (p && p->is_marker_chain() && i >= 0 && i < p->num_observations) ? p->time_index[i] : -1; }
int32_t rsba_problem_marker_idx(const rsba_problem* p, int64_t i) { return (p && p->is_marker_chain() && i >= 0 && i < p->num_observations) ? p->marker_index[i] : -1; }
double* rsba_problem_camera_parameters(rsba_problem* p, int32_t c) { return (p && c >= 0 && c < p->num_cameras) ? p->parameters.data() + 6 * c : nullptr; }
double* rsba_problem_marker_transform(rsba_problem* p, int32_t m) {
  return (p && p->is_marker_chain() && m >= 0 && m < p->num_markers) ? p->parameters.data() + 6 * (p->num_cameras + p->num_times + m) : nullptr;
}
int rsba_problem_point3d_coordinates(const rsba_problem* p, double* out) {
  if (!p || !out || !p->is_marker_chain()) return RSBA_ERR_ARG;
  rsba::MarkerCorners3d(*p, out);
  return RSBA_OK;
}

void rsba_options_default(rsba_options* o) {
  if (!o) return;
  memset(o, 0, sizeof(*o));
  o->max_num_iterations = 50; o->max_num_consecutive_invalid_steps = 5; o->jacobi_scaling = 1; o->minimizer_progress_to_stdout = 0;
  o->initial_trust_region_radius = 1e4; o->max_trust_region_radius = 1e16; o->min_trust_region_radius = 1e-32;
  o->min_relative_decrease = 1e-3; o->min_lm_diagonal = 1e-6; o->max_lm_diagonal = 1e32;
  o->function_tolerance = 1e-6; o->gradient_tolerance = 1e-10; o->parameter_tolerance = 1e-8; o->huber_delta = 0.0;
  o->device = -1; o->schur_impl = 1; o->profile_kernels = 0; o->rank = 0; o->world_size = 1; o->comm_unique_id = nullptr; o->stream = nullptr;
  o->max_solver_time_in_seconds = 1e9;
}

void rsba_evaluate_options_default(rsba_evaluate_options* o) {
  if (!o) return;
  memset(o, 0, sizeof(*o));
  o->apply_loss_function = 1;
}

int rsba_read_intrinsics_xml(const char* path, double* out4) { return rsba::ReadIntrinsicsXml(path, out4); }
int rsba_read_intrinsics_xml_dist(const char* path, double* out4, double* out5) { return rsba::ReadIntrinsicsXmlDist(path, out4, out5); }
int rsba_undistort_points(int32_t n, const double* image_points, const double* intrinsics4, const double* dist5, double* out) {
  return rsba::UndistortPoints(n, image_points, intrinsics4, dist5, out);
}
int rsba_write_outputs(rsba_problem* p, const char* xml, const char* dir, const char* p3d) {
  if (!p) return RSBA_ERR_ARG;
  return rsba::WriteOutputs(*p, xml, dir, p3d);
}

}  // extern "C"
