// hip_local_mapping.h -- C++ host mirror of SLAM_PIPELINE::LocalMapping::CreateNewMapPoints
// (slam_pipeline/src/LocalMapping.cc:136-294) above the C ABI: the current key frame's slot and view and the neighbours'
// slots and views in, the new map points out, in the order in which the reference creates them (neighbour by neighbour,
// match by match).
//
// The reference calls MatchFrames(current, KF_i) once per neighbour and triangulates each list match by match on one CPU
// thread.  Here msf_create_map_points (include/msf_local_mapping.h) matches the stored frames in one launch sequence and
// triangulates every list in one kernel behind it; the lists come back with the accepted points (for kp1 / kp2).
// Header-only and OpenCV-free, like hip_initializer.h: a view is an msf_view (GetRotation(), GetTranslation(), fx() ..
// cy()), a key point two integers, a map point three floats.  What stays with the caller: the baseline / median-depth
// gate (:166-174) -- leave the neighbours it drops out of `neighbours` -- and what follows an accepted point (MapPoint,
// AddObservation, AddMapPoint, UpdateNormalAndDepth; :267-278).  See INTEGRATION.md.
#pragma once

#include <cstdint>
#include <vector>

#include "hip_mirror_types.h"
#include "msf_local_mapping.h"

namespace msf {

struct Neighbour {   // vpNeighKFs[i]: where msf_store_frame put its image, and its pose
  int32_t slot;
  msf_view view;
};

struct NewMapPoint {
  int32_t neighbour;    // index into `neighbours`
  int32_t match;        // ikp: index into that neighbour's match list
  int32_t kp1[2];       // matchResult.keyPoints1[ikp] (current key frame)
  int32_t kp2[2];       // matchResult.keyPoints2[ikp] (the neighbour)
  Point3f x3D;
};

// CreateNewMapPoints' loop.  `handle`: the matcher the key frames were stored in with msf_store_frame; at most
// max_batch_pairs neighbours per call; `minParallax`: LocalMapping::mMinParallax (compared with the cosine, as the
// reference does; SlamParameters: 1.1).  `cap`: matches kept per neighbour.  Appends nothing and returns false when the
// call fails (msf_last_error(handle) has the text); a neighbour whose match list has no valid result (MSF_ERR_CAPACITY)
// contributes nothing and the others are kept, as a failed MatchFrames would leave an empty list.
inline bool NewMapPoints(msf_handle* handle, int32_t current_slot, const msf_view& current_view,
                         const std::vector<Neighbour>& neighbours, double minParallax, std::vector<NewMapPoint>& created,
                         int32_t cap = 4096) {
  created.clear();
  const size_t n = neighbours.size();
  if (!handle || cap < 1) return false;
  if (n == 0) return true;
  std::vector<int32_t> slots(n), num(n), n_new(n);
  std::vector<msf_view> views(n);
  for (size_t i = 0; i < n; i++) {
    slots[i] = neighbours[i].slot;
    views[i] = neighbours[i].view;
  }
  std::vector<msf_match> matches(n * static_cast<size_t>(cap));
  std::vector<msf_new_point> packed(n * static_cast<size_t>(cap));
  msf_new_points_params prm = sized<msf_new_points_params>();
  prm.max_cos_parallax = minParallax;
  prm.chi2 = 5.991;
  msf_new_points_result out = sized<msf_new_points_result>();
  out.n_new = n_new.data();
  out.packed = packed.data();
  const int rc = msf_create_map_points(handle, current_slot, &current_view, static_cast<int32_t>(n), slots.data(),
                                       views.data(), &prm, num.data(), matches.data(), cap, &out);
  if (rc != MSF_OK && rc != MSF_ERR_CAPACITY) return false;
  for (size_t i = 0; i < n; i++) {
    const msf_match* list = matches.data() + i * static_cast<size_t>(cap);
    for (int32_t k = 0; k < n_new[i]; k++) {
      const msf_new_point& p = packed[i * static_cast<size_t>(cap) + k];
      const msf_match& m = list[p.match];
      created.push_back(NewMapPoint{static_cast<int32_t>(i), p.match, {m.x1, m.y1}, {m.x2, m.y2}, Point3f{p.x, p.y, p.z}});
    }
  }
  return true;
}

}  // namespace msf
