// C++ mirror of the reference's problem container, over the C ABI of librsba.so.
//
// Same class name, namespace and accessors as RSCalibration::BALProblem in
// /root/reference/Main_Calibration/bundle_adjustment.h:18-54 (loadFile, parameters, camera_parameters,
// marker_transform, mutable_*_from_*, getPoint3dCoordinates, ...), so that bundle_adjustment_manager.cpp
// compiles against it unchanged apart from the Ceres calls it no longer needs.  What is gone: the four
// templated reprojection functors (:56-343) — their arithmetic now runs in HIP kernels behind rsba_solve —
// and cv::Mat (intrinsics are {fx, fy, ppx, ppy} per camera).
#pragma once
#include <array>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../rsba.h"

namespace RSCalibration {

struct Point3d { double x, y, z; };
using Intrinsics = std::array<double, 4>;  // fx, fy, ppx, ppy  (K(0,0), K(1,1), K(0,2), K(1,2))
using DistCoeffs = std::array<double, 5>;  // k1, k2, p1, p2, k3  (the 5 x 1 distCoeffs of Intrinsics/{serial}.xml)

class BALProblem {
 public:
  BALProblem() = default;
  BALProblem(const BALProblem&) = delete;
  BALProblem& operator=(const BALProblem&) = delete;
  ~BALProblem() { rsba_problem_free(p_); }

  // bundle_adjustment.cpp:132-187.  The reference reads MARKER_SIDE and the intrinsics elsewhere; here they are
  // handed in because the functors that used to hold them are gone.  Returns false when the file cannot be
  // opened (as the reference does) or is malformed.
  // dist_coeffs: the reference's create(observations, marker_side, intrinsics, dist_coeffs) takes them per camera and drops them
  // (bundle_adjustment.h:117-118); here they are honoured (rsba_problem_set_distortion).  Empty: a pinhole camera, as before; else
  // one per camera.
  bool loadFile(const char* filename, double marker_side, const std::vector<Intrinsics>& intrinsics,
                int model = RSBA_MODEL_MARKER_CHAIN, const std::vector<DistCoeffs>& dist_coeffs = {}) {
    rsba_problem_free(p_);
    p_ = nullptr;
    std::vector<double> k;
    for (const auto& i : intrinsics) k.insert(k.end(), i.begin(), i.end());
    if (rsba_problem_load_correspondence(filename, model, marker_side, k.data(), &p_) != RSBA_OK) return false;
    if (dist_coeffs.empty()) return true;
    std::vector<double> d;
    for (const auto& i : dist_coeffs) d.insert(d.end(), i.begin(), i.end());
    if ((int)dist_coeffs.size() == num_cameras() && rsba_problem_set_distortion(p_, d.data()) == RSBA_OK) return true;
    rsba_problem_free(p_);
    p_ = nullptr;
    return false;
  }
  // Test1 BALProblem::LoadFile (Test1_BundleAdjustment/bundle_adjustmenter.cpp:55-85)
  bool LoadFile(const char* filename, const Intrinsics& intrinsics) {
    rsba_problem_free(p_);
    p_ = nullptr;
    return rsba_problem_load_points_file(filename, intrinsics.data(), &p_) == RSBA_OK;
  }

  int num_cameras() const { return rsba_problem_num_cameras(p_); }
  int num_times() const { return rsba_problem_num_times(p_); }
  int num_observations() const { return (int)rsba_problem_num_observations(p_); }
  int num_observations_per_time_camera(int time_idx, int camera_idx) const { return rsba_problem_num_observations_per_time_camera(p_, time_idx, camera_idx); }
  const double* observations() const { return rsba_problem_observations(p_); }
  int num_parameters() const { return (int)rsba_problem_num_parameters(p_); }
  const double* parameters() const { return rsba_problem_parameters(p_); }
  int camera_idx(int observation_id) const { return rsba_problem_camera_idx(p_, observation_id); }
  int marker_idx(int observation_id) const { return rsba_problem_marker_idx(p_, observation_id); }
  double* camera_parameters(int camera_idx) { return rsba_problem_camera_parameters(p_, camera_idx); }
  double* marker_transform(int marker_idx) { return rsba_problem_marker_transform(p_, marker_idx); }
  double* mutable_camera_transform_from_base_camera(int i) { return rsba_problem_parameters(p_) + 6 * rsba_problem_camera_idx(p_, i); }
  double* mutable_base_marker_transform_from_base_camera(int i) { return rsba_problem_parameters(p_) + 6 * num_cameras() + 6 * rsba_problem_time_idx(p_, i); }
  double* mutable_marker_transform_from_base_marker(int i) { return rsba_problem_parameters(p_) + 6 * num_cameras() + 6 * num_times() + 6 * rsba_problem_marker_idx(p_, i); }
  // per-observation weights (ceres::ScaledLoss around each residual block's loss; rsba_problem_set_observation_weights): one
  // a_i >= 0 per observation, nullptr removes them / none set
  bool set_observation_weights(const double* weights) { return rsba_problem_set_observation_weights(p_, weights) == RSBA_OK; }
  const double* observation_weights() const { return rsba_problem_observation_weights(p_); }
  // lens distortion (rsba_problem_set_distortion): 5 per camera, nullptr removes them / none set
  bool set_distortion(const double* dist) { return rsba_problem_set_distortion(p_, dist) == RSBA_OK; }
  const double* distortion() const { return rsba_problem_distortion(p_); }
  // problem.AddParameterBlock(intrinsics_of_camera, 6) handed to the functor, with a SubsetParameterization for what stays fixed
  // (rsba_problem_set_intrinsics_free): the listed components of the camera's (fx, fy, cx, cy, k1, k2), indices 0..5, are refined by
  // the solve; an empty list makes them constants again.  False for a camera or an index out of range.  After a solve, intrinsics()
  // and distortion() hold the refined values.
  bool SetIntrinsicsFree(int camera_idx, const std::vector<int>& free_components) {
    int mask = 0;
    for (int q : free_components) { if (q < 0 || q > 5) return false; mask |= 1 << q; }
    return rsba_problem_set_intrinsics_free(p_, camera_idx, mask) == RSBA_OK;
  }
  // the camera's fx, fy, ppx, ppy (nullptr for a camera out of range)
  const double* intrinsics(int camera_idx) const {
    return camera_idx >= 0 && camera_idx < num_cameras() ? rsba_problem_intrinsics(p_) + 4 * camera_idx : nullptr;
  }
  // problem.SetParameterization(block, new ceres::SubsetParameterization(6, constant_parameters)) on a pose block handed out by the
  // mutable_* accessors above: the listed components of (rvec, tvec) are held (rsba_problem_set_parameter_subset_constant); an empty
  // list removes the subset.  False for a pointer that starts no pose block, an index outside 0..5 or all six components.
  bool SetSubsetConstant(double* block, const std::vector<int>& constant_parameters) {
    int mask = 0;
    for (int q : constant_parameters) { if (q < 0 || q > 5) return false; mask |= 1 << q; }
    return rsba_problem_set_parameter_subset_constant(p_, block - rsba_problem_parameters(p_), mask) == RSBA_OK;
  }
  // problem.AddResidualBlock(new ceres::NormalPrior(A, b), NULL, block) on a camera or marker block handed out by the mutable_*
  // accessors above (rsba_problem_set_block_prior): A 6 x 6 row-major, b 6; A = nullptr removes the prior.  False for a pointer that
  // starts no such block, a fixed base block, a time block or a non-finite value.
  bool SetNormalPrior(double* block, const double* A, const double* b) {
    return rsba_problem_set_block_prior(p_, block - rsba_problem_parameters(p_), A, b) == RSBA_OK;
  }
  // Test1 accessors
  // the start of the whole rig from its detections, on the GPU (rsba_problem_start_rig): the camera and time blocks by block resection
  // and propagation over the co-visibility graph; the marker blocks are inputs.  known (optional): num_cameras() + num_times() flags of
  // blocks that keep their values and serve from the first round.  status / rms (optional) are resized to that many entries.  Returns
  // the number of blocks left without a value (status 2 or 3), -1 when the call itself fails.  both_solutions
  // (RSBA_START_BOTH_SOLUTIONS): both poses of each candidate detection's planar marker are among a block's starts.
  int StartRig(const std::vector<uint8_t>* known = nullptr, int refine_sweeps = 1, int device = -1, std::vector<int32_t>* status = nullptr,
               std::vector<double>* rms = nullptr, bool both_solutions = false) {
    const size_t nb = (size_t)num_cameras() + (size_t)num_times();
    if (known && known->size() != nb) return -1;
    if (status) status->assign(nb, 0);
    if (rms) rms->assign(nb, 0.0);
    int32_t missing_times = 0, missing_cameras = 0;
    if (rsba_problem_start_rig2(p_, known ? known->data() : nullptr, refine_sweeps, device, both_solutions ? RSBA_START_BOTH_SOLUTIONS : 0u,
                                &missing_times, &missing_cameras, status ? status->data() : nullptr, rms ? rms->data() : nullptr) != RSBA_OK)
      return -1;
    return missing_times + missing_cameras;
  }
  // the start of a scene whose board geometry is not known (rsba_problem_start_scene): StartRig with the marker blocks fitted too, from the
  // base camera and the base marker alone.  known (optional): num_cameras() + num_times() + num_markers flags; status / rms (optional) are
  // resized to that many entries.  Returns the number of blocks left without a value (status 2 or 3), -1 when the call itself fails.
  // both_solutions: as for StartRig.
  int StartScene(const std::vector<uint8_t>* known = nullptr, int refine_sweeps = 1, int device = -1, std::vector<int32_t>* status = nullptr,
                 std::vector<double>* rms = nullptr, bool both_solutions = false) {
    const size_t nb = (size_t)num_cameras() + (size_t)num_times() + (size_t)rsba_problem_num_markers(p_);
    if (known && known->size() != nb) return -1;
    if (status) status->assign(nb, 0);
    if (rms) rms->assign(nb, 0.0);
    int32_t missing_times = 0, missing_cameras = 0, missing_markers = 0;
    if (rsba_problem_start_scene2(p_, known ? known->data() : nullptr, refine_sweeps, device, both_solutions ? RSBA_START_BOTH_SOLUTIONS : 0u,
                                  &missing_times, &missing_cameras, &missing_markers, status ? status->data() : nullptr,
                                  rms ? rms->data() : nullptr) != RSBA_OK)
      return -1;
    return missing_times + missing_cameras + missing_markers;
  }

  double* mutable_cameras() { return rsba_problem_parameters(p_); }
  double* mutable_points() { return rsba_problem_parameters(p_) + 6 * num_cameras(); }
  double* mutable_camera_for_observation(int i) { return mutable_cameras() + 6 * rsba_problem_camera_idx(p_, i); }
  double* mutable_point_for_observation(int i) { return mutable_points() + 3 * rsba_problem_point_idx(p_, i); }

  void getPoint3dCoordinates(std::vector<Point3d>& points) {
    std::vector<double> buf(12 * (size_t)num_observations());
    if (rsba_problem_point3d_coordinates(p_, buf.data()) != RSBA_OK) return;
    for (size_t i = 0; i < buf.size() / 3; ++i) points.push_back(Point3d{buf[3 * i], buf[3 * i + 1], buf[3 * i + 2]});
  }

  rsba_problem* handle() { return p_; }

 private:
  rsba_problem* p_ = nullptr;
};

}  // namespace RSCalibration
