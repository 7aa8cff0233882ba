// Launch interface of tracking_kernels.hip (Tracking::SearchLocalPoints around the matcher: the checking and owner
// pass, the frustum pass, the gate, the two claim passes), used by the entry points of include/msf_tracking.h in
// msf_abi.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "msf_tracking.h"
#include "tracking_solve.h"

namespace msf {

// Steps 1-2.  Required: status_word, n_to_match.  Everything else optional; null is skipped.
struct FrustumOut {
  int32_t* status_word;
  int32_t* n_to_match;
  uint8_t* status;
  uint8_t* visible;
  int32_t* owner_kf;
  float* u;
  float* v;
  float* dist;
  float* view_cos;
};

// What the gate writes besides n_to_match, for msf_search_local_points: train [n_kf] = slots [n_kf] or -1 for an
// unmatched key frame, matched [n_kf] = n_to_match > 0.  All null for the frustum entries.
struct GateOut {
  const int32_t* slots;
  int32_t* train;
  uint8_t* matched;
};

// The lists of step 4 as the matcher left them.
struct ClaimLists {
  const msf_match* matches;   // [n_kf][cap]
  int32_t cap;
  int32_t limit;              // a list's length is min(n_out, cap, limit)
  const int32_t* n_out;       // [n_kf]
  const uint8_t* matched;     // [n_kf]
};

// Steps 4-5.  Required: status_word, n_claims, n_claimed.  The correspondences are written iff all four are given.
struct ClaimOut {
  int32_t* status_word;
  int32_t* n_claims;
  int32_t* n_claimed;
  msf_local_claim* claims;
  uint8_t* claim_status;
  int32_t* n_corr;
  float* corr_p3d;
  float* corr_p2d;
  int32_t* corr_point;
  int32_t corr_cap;
};

// Clears the scratch's zeroed run, checks the map (s.bad) and takes the owner of every point.  Every call of the family
// starts with it.
hipError_t tracking_check(const tracking::Map& map, int width, int height, const tracking::Scratch& s, hipStream_t st);

// frustum pass + gate, behind tracking_check
hipError_t tracking_frustum(const tracking::Map& map, const tracking::Frustum& f, const tracking::Scratch& s,
                            const FrustumOut& out, const GateOut& gate, hipStream_t st);

// the two claim passes and the packing, behind tracking_check
hipError_t tracking_claims(const tracking::Map& map, int width, int height, const ClaimLists& in,
                           const tracking::Scratch& s, const ClaimOut& out, hipStream_t st);

}  // namespace msf
