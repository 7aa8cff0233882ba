// Launch interface of pnp_kernels.hip (PnPsolver's RANSAC iterations and Refine on every list of a batch), used by the
// msf_pnp_ransac* entry points in msf_abi.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "msf_pnp.h"

namespace msf {

// List l: p3d + l * cap * 3, p2d + l * cap * 2, length min(n[l], cap) (n == nullptr: one list of n_single
// correspondences); n[l] < 0 or a length below 4: no valid list.  sets [n_lists][n_iterations][4] or nullptr (drawn).
struct PnpLists {
  const float* p3d;
  const float* p2d;
  int32_t cap;
  const int32_t* n;
  int32_t n_single;
  const int32_t* sets;
};

struct PnpParams {
  float fx, fy, cx, cy;
  float th2;
  int32_t min_inliers;
  int32_t n_iterations;
  int32_t max_records;
  uint64_t seed;
};

// Device pointers laid out as msf_pnp_result says.  Required: n_records, counts, pose_f64 (the second launch reads the
// first one's counts and poses).  Everything else optional.
struct PnpOut {
  int32_t* n_records;
  int32_t* counts;
  int32_t* iteration;
  int32_t* n_inliers;
  int32_t* refined_ok;
  int32_t* n_refined;
  float* tcw_best;
  float* tcw_refined;
  uint8_t* inliers_best;
  uint8_t* inliers_refined;
  int32_t* sets;
  double* pose_f64;
  double* cws;
  double* ut_tail;
  double* betas;
  double* rep_errors;
  double* pca;
  double* rec_pose_f64;
  double* rec_cws;
  double* rec_ut_tail;
  double* rec_betas;
  double* rec_rep_errors;
  double* rec_pca;
};

hipError_t pnp_ransac(int n_lists, const PnpLists& in, const PnpParams& prm, const PnpOut& out, hipStream_t st);

}  // namespace msf
