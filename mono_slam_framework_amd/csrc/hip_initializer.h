// hip_initializer.h -- C++ host mirror of SLAM_PIPELINE::Initializer::Initialize
// (slam_pipeline/include/Initializer.h, slam_pipeline/src/Initializer.cc:75-150) above the C ABI: one match list in,
// R21, t21, vP3D, vbTriangulated and the yes / no out -- what Tracking::MonocularInitialization (Tracking.cc:251) uses.
//
// The reference draws its RANSAC sets, runs FindHomography and FindFundamental on two CPU threads and reconstructs on
// one.  Here the list is uploaded once and msf_find_models_device + msf_reconstruct_device (include/msf_abi.h,
// include/msf_initializer.h) run back to back on the handle's stream, the second reading the models and their inlier flags
// where the first left them on the device; one copy brings the block back.  Header-only and OpenCV-free, like hip_keyframe_database.h: K is a row-major float[9] (the CV_32F mK), a match
// an msf_match (MatchFramesResult::keyPoints1 / keyPoints2), a map point three floats.  See INTEGRATION.md.
#pragma once

#include <cstdint>
#include <cstring>
#include <vector>

#include "hip_device_block.h"
#include "hip_mirror_types.h"
#include "msf_initializer.h"

namespace msf {

// Initializer(K, sigma, iterations) + Initialize(matchResult, R21, t21, vP3D, vbTriangulated, minTriangulated,
// minParallax).  `handle`: a handle of either kind (the call uses none of its matcher state); `seed` keys the draw of the
// RANSAC sets (the reference seeds from std::random_device: there is no sequence to match).  The calling thread's current
// HIP device must be the handle's (msf_config.device): the list and the results live in a block allocated here.
// Returns Initialize()'s bool; on false -- also for a list shorter than 8 or longer than 8192 matches and for a failed
// device call (msf_last_error(handle) has the text) -- the outputs are left as the reference leaves them: R21 / t21
// zeroed, the vectors untouched.
inline bool Initialize(msf_handle* handle, const std::vector<msf_match>& matches, const float K[9], float sigma,
                       int iterations, uint64_t seed, int minTriangulated, float minParallax, float R21[9],
                       float t21[3], std::vector<Point3f>& vP3D, std::vector<bool>& vbTriangulated) {
  std::memset(R21, 0, 9 * sizeof(float));
  std::memset(t21, 0, 3 * sizeof(float));
  const size_t n = matches.size();
  if (!handle || n < 8 || n > 8192 || iterations < 1) return false;
  const int32_t cap = static_cast<int32_t>(n), n_hyp = iterations;

  // one block: the list and its length, then the models the two calls hand on and what comes back
  struct View {
    msf_match* matches;
    int32_t* n;
    size_t inputs_end;
    msf_ransac_batch found;
    msf_motion_result out;
  };
  DeviceBlock mem;
  View dev, host;
  const auto layout = [&](Carver& c) {
    View v;
    v.matches = c.take<msf_match>(n);
    v.n = c.take<int32_t>(1);
    v.inputs_end = c.off;
    v.found = sized<msf_ransac_batch>();
    for (msf_ransac_result* r : {&v.found.homography, &v.found.fundamental}) {
      *r = sized<msf_ransac_result>();
      r->m21 = c.take<float>(static_cast<size_t>(n_hyp) * 9);
      r->scores = c.take<float>(n_hyp);
      r->best = c.take<int32_t>(1);
      r->best_inliers = c.take<uint8_t>(n);
    }
    v.out = sized<msf_motion_result>();
    v.out.ok = c.take<int32_t>(1);
    v.out.R21 = c.take<float>(9);
    v.out.t21 = c.take<float>(3);
    v.out.points = c.take<float>(n * 3);
    v.out.triangulated = c.take<uint8_t>(n);
    return v;
  };
  if (!mem.place(layout, &dev, &host)) return false;
  std::memcpy(host.matches, matches.data(), n * sizeof(msf_match));
  *host.n = cap;
  if (!mem.upload()) return false;

  if (msf_find_models_device(handle, 1, dev.matches, cap, dev.n, n_hyp, seed, sigma, &dev.found, nullptr) != MSF_OK)
    return false;
  msf_motion_params prm = sized<msf_motion_params>();
  std::memcpy(prm.K, K, 9 * sizeof(float));
  prm.sigma = sigma;
  prm.min_triangulated = minTriangulated;
  prm.min_parallax = minParallax;
  if (msf_reconstruct_device(handle, 1, dev.matches, cap, dev.n, n_hyp, &dev.found, &prm, &dev.out, nullptr) != MSF_OK)
    return false;

  if (!mem.download() || !*host.out.ok) return false;
  std::memcpy(R21, host.out.R21, 9 * sizeof(float));
  std::memcpy(t21, host.out.t21, 3 * sizeof(float));
  vP3D.resize(n);
  std::memcpy(vP3D.data(), host.out.points, n * sizeof(Point3f));
  vbTriangulated.assign(host.out.triangulated, host.out.triangulated + n);
  return true;
}

}  // namespace msf
