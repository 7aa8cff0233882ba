// Launch interface of ba_kernels.hip (Optimizer::LocalBundleAdjustment / BundleAdjustment on every problem of a
// batch), used by the msf_bundle_adjust* entry points in msf_abi.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ba_solve.h"
#include "msf_ba.h"

namespace msf {

// Problem i is problems[i]: its cameras start at cam0 of the camera arrays, its points at point0, its edges at edge0;
// edge_cam / edge_point are local to it.  n_cams < 0: no valid problem.
struct BaBatch {
  const msf_ba_problem* problems;
  const float* cam_tcw;
  const uint8_t* cam_fixed;
  const float* points;
  const int32_t* edge_cam;
  const int32_t* edge_point;
  const float* edge_obs;
  int64_t total_cams, total_points, total_edges;
  int32_t max_free_cams;
  const int32_t* stop;   // null: no stop word
};

// Device pointers laid out as msf_ba_result says (a problem's rows at its cam0 / point0 / edge0, its per-iteration
// blocks at 64 times that).  Required: status.
using BaOut = ba::Out;

// `scratch`: ba::layout() over the call's totals, placed on device memory.
hipError_t bundle_adjust(int n_problems, const BaBatch& in, const ba::Params& prm, const ba::Scratch& scratch,
                         const BaOut& out, hipStream_t st);

}  // namespace msf
