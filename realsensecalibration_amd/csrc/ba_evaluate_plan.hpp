// Host-side planning of rsba_solver_evaluate (ba_evaluate.hpp): the index structures its gradient kernels need beyond what the
// solver keeps.  Plain C++ without HIP, vectors in and vectors out (the pattern of ba_schur_plan.hpp): ba_solver.hip allocates and
// copies, tests/evaluate_plan_driver.cpp checks the contracts under the host sanitizers.
//
// Every gradient slot is the sum of its block's observations IN A FIXED ORDER, so that two calls return the same bits.  The kernels
// get that order from lists that name, block by block, the observations that reference the block, ascending:
//   point model    the camera-major index over the solver's point-major observation slots (the points need none: a point's
//                  observations are contiguous in pt_ptr)
//   marker chain   per block of [C | T | M] the (observation, slot) pairs, slot = 0 camera, 1 time, 2 marker: where the block's six
//                  values sit in the observation's J'r (18 values, camera | time | marker)
// and from the mask of the blocks whose slots are 0.0 by definition: constant blocks, blocks no residual references, and the fixed
// base blocks of the marker-chain models (which no residual references as parameters).
#pragma once
#include <cstdint>
#include <vector>

#include "ba_problem.hpp"

namespace rsba {

// Which blocks' gradient slots are computed (1) and which are 0.0 by definition (0: constant or referenced by no residual).  Point
// model: the C cameras, then the P points in the problem's order.  camera_constant / point_constant may be shorter than C / P
// (missing entries: free), as rsba_problem keeps them.  The kernels place block b themselves: camera c at 6 c, point j at 6 C + 3 j.
std::vector<unsigned char> EvalPointLive(int C, int P, int64_t N, const int32_t* camera_index, const int32_t* point_index,
                                         const std::vector<uint8_t>& camera_constant, const std::vector<uint8_t>& point_constant);

// Camera-major index over the solver's observation slots.  `order[s]` is the problem observation in slot s (the solver's `order`),
// `pt_perm` the solver's point order (device position -> problem point; empty: identity).  Camera c owns entries
// [ptr[c], ptr[c + 1]): `slot` ascending, `point` the DEVICE position of the slot's point.
struct EvalCameraIndex {
  std::vector<int> ptr, slot, point;
};
EvalCameraIndex BuildEvalCameraIndex(int C, int P, const std::vector<int64_t>& order, const int32_t* camera_index,
                                     const int32_t* point_index, const std::vector<int>& pt_perm);

// Marker-chain models: one row per observation in the problem's order, the blocks of [C | T | M] it names as PARAMETERS (-1: the
// functor has no such block — camera 0, and marker 0 of RSBA_MODEL_MARKER_CHAIN) and the camera whose intrinsics project it.
// (The covariance reads the same rows in time order: ba_covariance_plan.hpp's CovMcRow is this struct.)
struct EvalMarkerRow {
  int cam_block, time_block, marker_block, camera;
};
inline EvalMarkerRow EvalMarkerRowOf(const rsba_problem& p, int64_t i) {
  return EvalMarkerRow{p.uses_camera(i) ? p.camera_block(i) : -1, p.time_block(i), p.uses_marker(i) ? p.marker_block(i) : -1, p.camera_index[i]};
}
inline std::vector<EvalMarkerRow> EvalMarkerRows(const rsba_problem& p) {
  std::vector<EvalMarkerRow> rows((size_t)p.num_observations);
  for (int64_t i = 0; i < p.num_observations; ++i) rows[i] = EvalMarkerRowOf(p, i);
  return rows;
}
// Block b owns entries [ptr[b], ptr[b + 1]): `obs` ascending; `slot` 0 / 1 / 2.  An observation is in the list of every block it names.
struct EvalMarkerLists {
  std::vector<int> ptr, obs;
  std::vector<unsigned char> slot;
};
EvalMarkerLists BuildEvalMarkerLists(int num_blocks, const std::vector<EvalMarkerRow>& rows);
// ... and the live mask of the blocks of [C | T | M] (block b sits at 6 b).  block_constant may be shorter than num_blocks.
std::vector<unsigned char> EvalMarkerLive(int num_blocks, const std::vector<EvalMarkerRow>& rows, const std::vector<uint8_t>& block_constant);

// ---- a marker-chain solver with free intrinsics under the extended layout (rsba_solver_set_extended_layout): the gradient has C more
// blocks behind [C | T | M], camera k's fx fy cx cy k1 k2 at block num_blocks + k.  k_eval_marker_intr writes observation i's pose
// J'r at obs_grad[18 i ..] as k_eval_marker does and its six intrinsics values at obs_grad[18 N + 6 i ..], behind all of them; the
// sum kernel (k_eval_marker_block_sum, unchanged) reads the six values at 18 obs + 6 slot, so the entry of observation i in an
// intrinsics block's list is (obs, slot) = (N + i / 3, i % 3): 18 (N + i / 3) + 6 (i % 3) = 18 N + 6 i.
struct EvalMarkerIntrPlan {
  EvalMarkerLists lists;              // num_blocks + C lists: the pose blocks' as BuildEvalMarkerLists gives them, then a camera's detections, ascending
  std::vector<unsigned char> live;    // num_blocks + C: an intrinsics block is live when its mask is not 0 and an observation names the camera
  std::vector<unsigned char> held;    // num_blocks + C: per live block the components written as 0.0 — a pose block's subset mask, an intrinsics
                                      // block's clear mask bits; 0 for a block that is not live (all of its slots are 0.0 already)
};
// block_constant / block_subset / intr_mask may be shorter than their counts (missing entries: free / no mask / mask 0).
EvalMarkerIntrPlan PlanEvalMarkerIntr(int num_blocks, int C, const std::vector<EvalMarkerRow>& rows, const std::vector<uint8_t>& block_constant,
                                      const std::vector<uint8_t>& block_subset, const std::vector<int>& intr_mask);

// ---- the Jacobian of rsba_solver_evaluate_jacobian, in compressed-row form (ba_evaluate_jacobian.hpp)
// Rows in the problem's observation order (2 per observation on the point model, 8 on the marker chain), columns = parameter
// offsets.  A row holds every column of every block its observation names as a parameter and that is not constant — camera, then
// point / camera, time, marker: ascending offsets — so all rows of an observation have the same width and its values are one
// contiguous piece, row after row: `off[i]` is where observation i's piece starts (off[N]: the number of nonzeros), `width[i]` the
// entries per row.  A named block is referenced by definition, so of EvalPointLive / EvalMarkerLive only the constant part applies.
struct EvalJacobianLayout {
  std::vector<int64_t> off;           // N + 1
  std::vector<unsigned char> width;   // N: 0, 3, 6 or 9 (point model); 0, 6, 12 or 18 (marker chain)
};
EvalJacobianLayout EvalPointJacobianLayout(int64_t N, const int32_t* camera_index, const int32_t* point_index,
                                           const std::vector<uint8_t>& camera_constant, const std::vector<uint8_t>& point_constant);
EvalJacobianLayout EvalMarkerJacobianLayout(const std::vector<EvalMarkerRow>& rows, const std::vector<uint8_t>& block_constant);
// row_ptr (rows_per_obs N + 1 entries) from the layout alone.  The three fill functions do nothing for a nullptr output.
void EvalJacobianRowPtr(const EvalJacobianLayout& l, int rows_per_obs, int64_t* row_ptr);
// cols (off[N] entries) of the two models, the same walk as the layout's.  Written into the caller's array: at two million
// observations it is 36 million entries, which nobody wants to hold twice.
void EvalPointJacobianCols(const EvalJacobianLayout& l, int C, const int32_t* camera_index, const int32_t* point_index,
                           const std::vector<uint8_t>& camera_constant, const std::vector<uint8_t>& point_constant, int32_t* cols);
void EvalMarkerJacobianCols(const EvalJacobianLayout& l, const std::vector<EvalMarkerRow>& rows, const std::vector<uint8_t>& block_constant,
                            int32_t* cols);
// Point model: what the kernel gathers through, one entry per observation in the problem's order — its camera and the DEVICE
// position of its point (pt_perm: device position -> problem point; empty: identity).
struct EvalJacobianPointRow {
  int32_t camera, point;
};
std::vector<EvalJacobianPointRow> EvalJacobianPointRows(int P, int64_t N, const int32_t* camera_index, const int32_t* point_index,
                                                        const std::vector<int>& pt_perm);

}  // namespace rsba
