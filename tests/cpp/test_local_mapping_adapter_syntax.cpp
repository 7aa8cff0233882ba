// Syntax-only translation unit for tests/test_local_mapping_adapter_syntax.py: csrc/hip_local_mapping.h instantiated the
// way LocalMapping::CreateNewMapPoints would call it (slam_pipeline/src/LocalMapping.cc:136-294), with no OpenCV type in
// sight, and next to hip_initializer.h (the two share msf::Point3f).
#include <vector>

#include "hip_initializer.h"
#include "hip_local_mapping.h"

size_t create_new_map_points(msf_handle* h, const msf_view& current, const std::vector<msf::Neighbour>& neighbours) {
  std::vector<msf::NewMapPoint> created;
  if (!msf::NewMapPoints(h, 0, current, neighbours, 1.1, created)) return 0;
  if (!msf::NewMapPoints(h, 0, current, neighbours, 1.1, created, 2048)) return 0;
  float sum = 0.f;
  for (const msf::NewMapPoint& p : created) sum += p.x3D.x + p.x3D.y + p.x3D.z + (float)(p.kp1[0] + p.kp2[1] + p.neighbour + p.match);
  return created.size() + (sum > 0.f ? 1 : 0);
}
