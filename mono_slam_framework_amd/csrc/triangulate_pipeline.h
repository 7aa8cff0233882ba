// Launch interface of triangulate_kernels.hip (the loop body of LocalMapping::CreateNewMapPoints on every match of
// every list), used by the msf_new_points* / msf_create_map_points entry points in msf_abi.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "msf_local_mapping.h"

namespace msf {

// The lists as the matcher leaves them: list l is matches + l * cap, its length min(n_out[l], cap, limit)
// (n_out == nullptr: one list of n_single matches); n_out[l] < 0: no valid list.  view1 / view2 [n_lists].
struct NewPointLists {
  const msf_match* matches;
  int32_t cap;
  int32_t limit;
  const int32_t* n_out;
  int32_t n_single;
  const msf_view* view1;
  const msf_view* view2;
};

struct NewPointParams {
  double max_cos;   // LocalMapping::mMinParallax, compared with the cosine
  double chi2;      // 5.991
};

// Every array has a leading [n_lists] and the lists' stride `cap`.  Required: n_new.  Optional: packed [cap],
// status [cap], points [cap][3], hom [cap][4], cos_parallax [cap].
struct NewPointOut {
  int32_t* n_new;
  msf_new_point* packed;
  uint8_t* status;
  float* points;
  float* hom;
  double* cos_parallax;
};

hipError_t new_points(int n_lists, const NewPointLists& in, const NewPointParams& prm, const NewPointOut& out,
                      hipStream_t st);

}  // namespace msf
