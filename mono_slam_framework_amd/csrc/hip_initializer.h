// hip_initializer.h -- C++ host mirror of SLAM_PIPELINE::Initializer::Initialize
// (slam_pipeline/include/Initializer.h, slam_pipeline/src/Initializer.cc:75-150) above the C ABI: one match list in,
// R21, t21, vP3D, vbTriangulated and the yes / no out -- what Tracking::MonocularInitialization (Tracking.cc:251) uses.
//
// The reference draws its RANSAC sets, runs FindHomography and FindFundamental on two CPU threads and reconstructs on
// one.  Here the list is uploaded once and msf_find_models_device + msf_reconstruct_device (include/msf_abi.h,
// include/msf_initializer.h) run back to back on the handle's stream; the models and their inlier flags never leave the
// device.  Header-only and OpenCV-free, like hip_keyframe_database.h: K is a row-major float[9] (the CV_32F mK), a match
// an msf_match (MatchFramesResult::keyPoints1 / keyPoints2), a map point three floats.  See INTEGRATION.md.
#pragma once

#ifndef __HIP_PLATFORM_AMD__
#define __HIP_PLATFORM_AMD__ 1
#endif
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <cstring>
#include <vector>

#include "msf_initializer.h"

namespace msf {

#ifndef MSF_POINT3F_DEFINED   // hip_local_mapping.h has the same type
#define MSF_POINT3F_DEFINED
struct Point3f {   // cv::Point3f
  float x, y, z;
};
#endif

namespace detail {
// one device block, carved into 256-byte aligned pieces; freed on scope exit
class DeviceArena {
 public:
  DeviceArena() = default;
  DeviceArena(const DeviceArena&) = delete;
  DeviceArena& operator=(const DeviceArena&) = delete;
  ~DeviceArena() {
    if (base_) hipFree(base_);
  }
  size_t reserve(size_t bytes) {
    const size_t at = size_;
    size_ += (bytes + 255) & ~static_cast<size_t>(255);
    return at;
  }
  bool allocate() {
    const size_t bytes = size_ ? size_ : 256;
    return hipMalloc(&base_, bytes) == hipSuccess && hipMemset(base_, 0, bytes) == hipSuccess;
  }
  template <class T>
  T* at(size_t offset) const { return reinterpret_cast<T*>(static_cast<char*>(base_) + offset); }

 private:
  void* base_ = nullptr;
  size_t size_ = 0;
};
}  // namespace detail

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

  detail::DeviceArena mem;
  const size_t o_matches = mem.reserve(n * sizeof(msf_match)), o_n = mem.reserve(sizeof(int32_t));
  size_t o_m21[2], o_scores[2], o_best[2], o_inl[2];
  for (int m = 0; m < 2; m++) {
    o_m21[m] = mem.reserve(static_cast<size_t>(n_hyp) * 9 * sizeof(float));
    o_scores[m] = mem.reserve(static_cast<size_t>(n_hyp) * sizeof(float));
    o_best[m] = mem.reserve(sizeof(int32_t));
    o_inl[m] = mem.reserve(n);
  }
  const size_t o_ok = mem.reserve(sizeof(int32_t)), o_R = mem.reserve(9 * sizeof(float));
  const size_t o_t = mem.reserve(3 * sizeof(float)), o_pts = mem.reserve(n * sizeof(Point3f)), o_tri = mem.reserve(n);
  if (!mem.allocate()) return false;
  if (hipMemcpy(mem.at<msf_match>(o_matches), matches.data(), n * sizeof(msf_match), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(mem.at<int32_t>(o_n), &cap, sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess)
    return false;

  msf_ransac_batch found;
  std::memset(&found, 0, sizeof found);
  found.struct_size = sizeof found;
  msf_ransac_result* res[2] = {&found.homography, &found.fundamental};
  for (int m = 0; m < 2; m++) {
    res[m]->struct_size = sizeof(msf_ransac_result);
    res[m]->m21 = mem.at<float>(o_m21[m]);
    res[m]->scores = mem.at<float>(o_scores[m]);
    res[m]->best = mem.at<int32_t>(o_best[m]);
    res[m]->best_inliers = mem.at<uint8_t>(o_inl[m]);
  }
  if (msf_find_models_device(handle, 1, mem.at<msf_match>(o_matches), cap, mem.at<int32_t>(o_n), n_hyp, seed, sigma,
                             &found, nullptr) != MSF_OK)
    return false;

  msf_motion_params prm;
  std::memset(&prm, 0, sizeof prm);
  prm.struct_size = sizeof prm;
  std::memcpy(prm.K, K, 9 * sizeof(float));
  prm.sigma = sigma;
  prm.min_triangulated = minTriangulated;
  prm.min_parallax = minParallax;
  msf_motion_result out;
  std::memset(&out, 0, sizeof out);
  out.struct_size = sizeof out;
  out.ok = mem.at<int32_t>(o_ok);
  out.R21 = mem.at<float>(o_R);
  out.t21 = mem.at<float>(o_t);
  out.points = mem.at<float>(o_pts);
  out.triangulated = mem.at<uint8_t>(o_tri);
  if (msf_reconstruct_device(handle, 1, mem.at<msf_match>(o_matches), cap, mem.at<int32_t>(o_n), n_hyp, &found, &prm,
                             &out, nullptr) != MSF_OK)
    return false;

  int32_t ok = 0;
  if (hipMemcpy(&ok, out.ok, sizeof ok, hipMemcpyDeviceToHost) != hipSuccess || !ok) return false;
  std::vector<Point3f> points(n);
  std::vector<uint8_t> flags(n);
  if (hipMemcpy(R21, out.R21, 9 * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(t21, out.t21, 3 * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(points.data(), out.points, n * sizeof(Point3f), hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(flags.data(), out.triangulated, n, hipMemcpyDeviceToHost) != hipSuccess) {
    std::memset(R21, 0, 9 * sizeof(float));
    std::memset(t21, 0, 3 * sizeof(float));
    return false;
  }
  vP3D.swap(points);
  vbTriangulated.assign(flags.begin(), flags.end());
  return true;
}

}  // namespace msf
