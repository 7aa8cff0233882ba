// Launch interface of pose_kernels.hip (Optimizer::PoseOptimization on every list of a batch), used by the
// msf_pose_optimize* entry points in msf_abi.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "msf_pose.h"

namespace msf {

// List l: p3d + l * cap * 3, p2d + l * cap * 2, length min(n[l], cap) (n == nullptr: one list of n_single
// correspondences); n[l] < 0: no valid list.  Its entry pose: tcw0 + l * tcw0_stride (12 floats); its mask:
// mask + l * mask_stride (bytes), or every correspondence when mask == nullptr.
struct PoseLists {
  const float* p3d;
  const float* p2d;
  int32_t cap;
  const int32_t* n;
  int32_t n_single;
  const float* tcw0;
  int64_t tcw0_stride;
  const uint8_t* mask;
  int64_t mask_stride;
};

struct PoseParams {
  float fx, fy, cx, cy;
  float chi2;
};

// Device pointers laid out as msf_pose_result says.  Required: n_good.  Everything else optional.
struct PoseOut {
  int32_t* n_good;
  float* tcw;
  uint8_t* outliers;
  int32_t* n_edges;
  int32_t* rounds_run;
  double* pose_f64;
  double* round_pose_f64;
  int32_t* round_n_bad;
  int32_t* round_iterations;
  int32_t* it_trials;
  double* it_lambda_in;
  double* it_lambda_out;
  double* it_cost_in;
  double* it_cost_out;
  double* it_H;
  double* it_b;
  double* it_pose_out;
};

hipError_t pose_optimize(int n_lists, const PoseLists& in, const PoseParams& prm, const PoseOut& out, hipStream_t st);

}  // namespace msf
