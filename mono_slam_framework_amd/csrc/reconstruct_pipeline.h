// Launch interface of reconstruct_kernels.hip (the tail of Initializer::Initialize: pose and map points from the kept
// H / F of every match list), used by the msf_reconstruct* entry points in msf_abi.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "msf_abi.h"

namespace msf {

constexpr int kMaxReconstructMatches = 8192;   // one 64-bit key per match in LDS

// Initializer(K, sigma) + Initialize(..., minTriangulated, minParallax)
struct MotionParams {
  float K[9];
  float th2;   // 4 sigma^2
  int32_t min_triangulated;
  float min_parallax;
};

// The lists and their models, as msf_find_models_device leaves them: list l is matches + l * cap, its length
// min(n_out[l], cap) (n_out == nullptr: one list of n_single matches).  Index 0: homography, 1: fundamental.
// m21 [n_lists][n_hyp][9], scores [n_lists][n_hyp], best [n_lists], inliers [n_lists][cap].
// forced_model >= 0: reconstruct from that model's hypothesis 0 whatever the scores (best and scores are not read).
struct MotionLists {
  const msf_match* matches;
  int32_t cap;
  const int32_t* n_out;
  int32_t n_single;
  int32_t n_hyp;
  int32_t forced_model;
  const float* m21[2];
  const float* scores[2];
  const int32_t* best[2];
  const uint8_t* inliers[2];
};

// Every array has a leading [n_lists].  Required: model, n_inliers, n_cand, cand_R [8][9], cand_t [8][3], cand_good [8],
// cand_parallax [8], winner, ok.  Optional: R21 [9], t21 [3], points [cap][3], triangulated [cap].
struct MotionOut {
  int32_t* model;
  int32_t* n_inliers;
  int32_t* n_cand;
  float* cand_R;
  float* cand_t;
  int32_t* cand_good;
  float* cand_parallax;
  int32_t* winner;
  int32_t* ok;
  float* R21;
  float* t21;
  float* points;
  uint8_t* triangulated;
};

hipError_t reconstruct_motion(int n_lists, const MotionLists& in, const MotionParams& prm, const MotionOut& out,
                              hipStream_t st);

}  // namespace msf
