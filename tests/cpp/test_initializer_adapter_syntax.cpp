// Syntax-only translation unit for tests/test_initializer_adapter_syntax.py: csrc/hip_initializer.h instantiated the way
// Tracking::MonocularInitialization would call it (slam_pipeline/src/Tracking.cc:251), with no OpenCV type in sight.
#include <vector>

#include "hip_initializer.h"

bool initialize_once(msf_handle* h, const std::vector<msf_match>& matches) {
  const float K[9] = {500.f, 0.f, 320.f, 0.f, 500.f, 240.f, 0.f, 0.f, 1.f};
  float R21[9], t21[3];
  std::vector<msf::Point3f> vP3D;
  std::vector<bool> vbTriangulated;
  return msf::Initialize(h, matches, K, 1.0f, 200, 0x1234u, 50, 1.0f, R21, t21, vP3D, vbTriangulated) &&
         vP3D.size() == vbTriangulated.size();
}
