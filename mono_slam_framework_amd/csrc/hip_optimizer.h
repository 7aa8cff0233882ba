// hip_optimizer.h -- C++ host mirror of SLAM_PIPELINE::Optimizer::PoseOptimization (slam_pipeline/include/Optimizer.h,
// slam_pipeline/src/Optimizer.cc:217-334) above the C ABI: the four Levenberg-Marquardt rounds and the chi2 flags are
// msf_pose_optimize / msf_pose_optimize_device (include/msf_pose.h).
//
// The reference walks pFrame->mKeyPointMap, adds one edge per key point that has a map point, optimises, and writes
// the flags (SetOutlier, :312-316) and the pose (SetPose, :331) back into the frame.  Here the caller gathers what the
// edges are made of -- GetWorldPos() of each map point and the key point's pixel, in the order of its own index list --
// and gets back the flags in that order, the pose in place and the return value nInitialCorrespondences - nBad.
// With fewer than 3 correspondences the return is 0, the pose is untouched and every flag is false (:253, :285).
//
// Tracking::Relocalization (Tracking.cc:827) calls PoseOptimization once per candidate on PnPsolver's output:
// PoseOptimizationBatch runs all candidates in ONE msf_pose_optimize_device call.
//
// Header-only and OpenCV-free, like hip_pnp_solver.h: a 3-D point is three floats, a pixel two, Tcw a row-major
// float[16].  See INTEGRATION.md.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "hip_device_block.h"
#include "hip_mirror_types.h"
#include "msf_pose.h"

namespace msf {

class Optimizer {
 public:
  // intrinsics = (fx, fy, cx, cy) of the frame; Tcw in: pFrame->mTcw, out: the optimised pose (rows 0..2 replaced, row 3
  // set to 0 0 0 1, as Converter::toCvMat builds it); outliers[i]: mKeyPointMap.IsOutlier of correspondence i afterwards.
  // -> nInitialCorrespondences - nBad; -1: the call failed and msf_last_error(handle) has the text (Tcw and outliers are
  // left alone).
  static int PoseOptimization(msf_handle* handle, const std::vector<Point3f>& points, const std::vector<Point2f>& pixels,
                              const float intrinsics[4], float Tcw[16], std::vector<bool>& outliers, float chi2 = 5.991f) {
    const int32_t n = static_cast<int32_t>(std::min(points.size(), pixels.size()));
    const msf_pose_params prm = Params(intrinsics, chi2);
    int32_t n_good = 0, rounds = 0;
    float optimised[12];
    std::vector<uint8_t> flags(n > 0 ? n : 1, 0);
    msf_pose_result out = sized<msf_pose_result>();
    out.n_good = &n_good, out.rounds_run = &rounds, out.Tcw = optimised, out.outliers = flags.data();
    const int rc = msf_pose_optimize(handle, n, n ? &points[0].x : nullptr, n ? &pixels[0].x : nullptr, Tcw, nullptr, &prm, &out);
    if (rc != MSF_OK) return -1;
    Report(n, flags.data(), rounds, optimised, Tcw, outliers);
    return n_good;
  }

  // One candidate of a batch: what PoseOptimization takes and gives, n_good its return.
  struct Candidate {
    const std::vector<Point3f>* points;
    const std::vector<Point2f>* pixels;
    float* Tcw;                   // [16], in-out
    std::vector<bool>* outliers;  // out
    int n_good;                   // out
  };

  // PoseOptimization of every candidate with ONE msf_pose_optimize_device call on a block allocated here.  The calling
  // thread's current HIP device must be the handle's.  false: a failed call (nothing is written).
  static bool PoseOptimizationBatch(msf_handle* handle, std::vector<Candidate>& candidates, const float intrinsics[4],
                                    float chi2 = 5.991f) {
    const size_t L = candidates.size();
    if (!L) return true;
    size_t cap = 1;
    for (const Candidate& c : candidates) cap = std::max(cap, std::min(c.points->size(), c.pixels->size()));
    // one block: the lists, their lengths and entry poses, then n_good, rounds_run, Tcw and the flags
    struct View {
      float *p3d, *p2d, *Tcw0;
      int32_t* n;
      size_t inputs_end;
      msf_pose_result out;
    };
    DeviceBlock mem;
    View dev, host;
    const auto layout = [&](Carver& c) {
      View v;
      v.p3d = c.take<float>(L * cap * 3);
      v.p2d = c.take<float>(L * cap * 2);
      v.n = c.take<int32_t>(L);
      v.Tcw0 = c.take<float>(L * 12);
      v.inputs_end = c.off;
      v.out = sized<msf_pose_result>();
      v.out.n_good = c.take<int32_t>(L);
      v.out.rounds_run = c.take<int32_t>(L);
      v.out.Tcw = c.take<float>(L * 12);
      v.out.outliers = c.take<uint8_t>(L * cap);
      return v;
    };
    if (!mem.place(layout, &dev, &host)) return false;
    for (size_t l = 0; l < L; l++) {
      const Candidate& c = candidates[l];
      const size_t n = std::min(c.points->size(), c.pixels->size());
      host.n[l] = static_cast<int32_t>(n);
      if (n) std::memcpy(host.p3d + l * cap * 3, c.points->data(), n * sizeof(Point3f));
      if (n) std::memcpy(host.p2d + l * cap * 2, c.pixels->data(), n * sizeof(Point2f));
      std::memcpy(host.Tcw0 + l * 12, c.Tcw, 48);
    }
    const msf_pose_params prm = Params(intrinsics, chi2);
    if (!mem.upload() ||
        msf_pose_optimize_device(handle, static_cast<int32_t>(L), dev.p3d, dev.p2d, static_cast<int32_t>(cap), dev.n,
                                 dev.Tcw0, 12, nullptr, 0, &prm, &dev.out, nullptr) != MSF_OK ||
        !mem.download())
      return false;
    for (size_t l = 0; l < L; l++) {
      Candidate& c = candidates[l];
      Report(host.n[l], host.out.outliers + l * cap, host.out.rounds_run[l], host.out.Tcw + l * 12, c.Tcw, *c.outliers);
      c.n_good = host.out.n_good[l];
    }
    return true;
  }

  // PoseOptimization of ONE list that is already in device memory -- d_p3d [cap][3], d_p2d [cap][2], its length at
  // *d_n -- as msf_search_local_points leaves the correspondences of a tracked frame with MSF_SEARCH_KEEP_ON_DEVICE
  // (hip_tracking.h: msf::TrackLocalMap).  Only the entry pose goes up and only the pose, the counts and the flags come
  // back, through a block allocated here.  -> as PoseOptimization; -1 also for a list without a valid length (*d_n < 0).
  static int PoseOptimizationDevice(msf_handle* handle, const float* d_p3d, const float* d_p2d, int32_t cap,
                                    const int32_t* d_n, const float intrinsics[4], float Tcw[16],
                                    std::vector<bool>& outliers, float chi2 = 5.991f) {
    if (cap < 1) return -1;
    struct View {
      float* Tcw0;
      size_t inputs_end;
      msf_pose_result out;
    };
    DeviceBlock mem;
    View dev, host;
    const auto layout = [&](Carver& c) {
      View v;
      v.Tcw0 = c.take<float>(12);
      v.inputs_end = c.off;
      v.out = sized<msf_pose_result>();
      v.out.n_good = c.take<int32_t>(1);
      v.out.rounds_run = c.take<int32_t>(1);
      v.out.n_edges = c.take<int32_t>(1);
      v.out.Tcw = c.take<float>(12);
      v.out.outliers = c.take<uint8_t>(cap);
      return v;
    };
    if (!mem.place(layout, &dev, &host)) return -1;
    std::memcpy(host.Tcw0, Tcw, 48);
    const msf_pose_params prm = Params(intrinsics, chi2);
    if (!mem.upload() ||
        msf_pose_optimize_device(handle, 1, d_p3d, d_p2d, cap, d_n, dev.Tcw0, 12, nullptr, 0, &prm, &dev.out, nullptr) != MSF_OK ||
        !mem.download() || host.out.n_good[0] < 0)
      return -1;
    Report(host.out.n_edges[0], host.out.outliers, host.out.rounds_run[0], host.out.Tcw, Tcw, outliers);
    return host.out.n_good[0];
  }

 private:
  static msf_pose_params Params(const float intrinsics[4], float chi2) {
    msf_pose_params prm = sized<msf_pose_params>();
    prm.fx = intrinsics[0], prm.fy = intrinsics[1], prm.cx = intrinsics[2], prm.cy = intrinsics[3];
    prm.chi2 = chi2;
    return prm;
  }

  // :312-333: the flags of every correspondence; the pose only when a round ran (:285 returns before SetPose)
  static void Report(int32_t n, const uint8_t* flags, int32_t rounds, const float* optimised, float Tcw[16],
                     std::vector<bool>& outliers) {
    outliers.assign(n, false);
    if (!rounds) return;
    for (int32_t i = 0; i < n; i++) outliers[i] = flags[i] != 0;
    std::memcpy(Tcw, optimised, 48);
    Tcw[12] = Tcw[13] = Tcw[14] = 0.0f;
    Tcw[15] = 1.0f;
  }
};

}  // namespace msf
