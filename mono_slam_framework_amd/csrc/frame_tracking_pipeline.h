// Launch interface of frame_tracking_kernels.hip (the body of Tracking::TrackWithMotionModel / TrackReferenceKeyFrame
// around k_pose_optimize: the check-and-carry launch and the cut), used by the entry points of
// include/msf_frame_tracking.h in msf_abi.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "frame_tracking_solve.h"
#include "msf_frame_tracking.h"

namespace msf {

// The one list of a call as the matcher left it, and the bounds of steps 1 and 3.
struct CarryIn {
  const msf_match* matches;   // [cap]
  int32_t cap;
  const int32_t* n_out;       // [1]
  int32_t min_matches;        // 0: no gate (msfx_carry_points_device)
  int32_t corr_cap;
  float tcw0[12];             // the entry pose by value: the carry puts it where the later launches read it
  float* tcw0_device;         // [12] in the workspace, or null (msfx_carry_points_device)
};

// Steps 2-3.  Every pointer non-null: the entry points put a piece of the workspace where the caller gave none.
struct CarryOut {
  int32_t* track_status;      // written by the carry only when `last`
  int32_t* n_map;
  msfx_frame_point* map;
  uint8_t* carry_status;
  uint8_t* cur_status;
  float* corr_p3d;
  float* corr_p2d;
  int32_t* corr_point;
};

// Steps 5-6.  Every pointer non-null.  pose_*: what k_pose_optimize wrote between the two launches.
struct CutIn {
  const float* tcw0;          // [12], device
  const float* pose_tcw;      // [12]
  const int32_t* pose_n_good; // [1]
  const uint8_t* outliers;    // [corr_cap]
  int32_t min_map_matches;
  const int32_t* n_out;       // [1]: the matcher's count, for the summary
};

struct CutOut {
  int32_t* track_status;
  const int32_t* n_map;
  msfx_frame_point* map;
  float* tcw;
  int32_t* n_good;
  int32_t* n_kept;
  int32_t* kept_key;
  int32_t* kept_point;
  int32_t* n_removed;
  msfx_removed_point* removed;
  int32_t* n_matches_map;
};

// One workgroup: the map checked, the gate, the candidates sorted in LDS, the winners packed in key order.  Leaves
// s.state for the launches behind it; `last`: no launch follows, track_status is written here.
hipError_t frame_tracking_carry(const ftrack::Map& map, int width, int height, const CarryIn& in, const ftrack::Scratch& s,
                                const CarryOut& out, bool last, hipStream_t st);

// One workgroup, behind frame_tracking_carry and pose_optimize (d_n = s.state + 1).
hipError_t frame_tracking_cut(const ftrack::Map& map, const CutIn& in, const ftrack::Scratch& s, const CutOut& out,
                              hipStream_t st);

}  // namespace msf
