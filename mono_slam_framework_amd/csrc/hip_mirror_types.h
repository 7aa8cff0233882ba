// hip_mirror_types.h -- what the header-only C++ mirrors (hip_initializer.h, hip_local_mapping.h, hip_pnp_solver.h,
// hip_optimizer.h, hip_tracking.h) share: the two point types and the zeroed, sized struct every C ABI call starts from.  No HIP and no
// OpenCV in here.
#pragma once

#include <cstring>

#define MSF_POINT3F_DEFINED   // the mirrors used to guard their own copies with these: still defined for whoever tests them
#define MSF_POINT2F_DEFINED

namespace msf {

struct Point3f {   // cv::Point3f
  float x, y, z;
};

struct Point2f {   // cv::Point2f
  float x, y;
};

// a params or result struct of the C ABI, all zero (every optional pointer NULL) and with its struct_size set
template <class S>
S sized() {
  S s;
  std::memset(&s, 0, sizeof s);
  s.struct_size = sizeof s;
  return s;
}

}  // namespace msf
