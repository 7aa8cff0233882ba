// hip_bundle_adjustment.h -- C++ host mirror of SLAM_PIPELINE::Optimizer::LocalBundleAdjustment
// (slam_pipeline/src/Optimizer.cc:336-574) and Optimizer::BundleAdjustment (:71-215) above the C ABI: the
// Schur-complement Levenberg-Marquardt rounds and the vToErase flags are msf_bundle_adjust_device (include/msf_ba.h).
//
// The reference collects its problem from the map, optimises and writes the result back into the map.  Here the caller
// collects the problem -- poses, which of them are fixed, points, and one edge per observation, sorted by point in the
// order in which the reference creates them -- and gets back the poses and points in place and one flag per edge.
// What stays with the caller, in the reference's order:
//
//   // :337-384  the covisibility walk: lLocalKeyFrames (pKF and GetVectorCovisibleKeyFrames(), !isBad()) are the free
//   //           cameras, lLocalMapPoints their map points (!isBad()), lFixedCameras the other observers of those
//   //           points; key frame 0 is fixed (:399).  For BundleAdjustment: every key frame and map point, key frame 0
//   //           fixed (:86), and a point without an edge is left out (:139-147).
//   msf::BundleAdjuster::Problem pb;
//   for (KeyFrame* kf : cameras) { push 16 floats of kf->GetPose() to pb.Tcw; pb.fixed.push_back(is_fixed(kf)); }
//   for (MapPoint* mp : points) {
//     pb.points.push_back(GetWorldPos());
//     for (auto& ob : mp->GetObservations())            // !pKFi->isBad()
//       pb.edges.push_back({index_of(ob.first), index_of(mp), pixel_of(ob.first, ob.second)});
//   }
//   msf::BundleAdjuster ba(handle, intrinsics);
//   if (!ba.LocalBundleAdjustment(pb, pbStopFlag_as_int32)) ...error...
//   // :530-548  for every edge with pb.outliers[e]: pKFi->EraseMapPointMatch(pMP); pMP->EraseObservation(pKFi);
//   // :551-572  for every free camera: pKF->SetPose(pb.Tcw of it); for every point: pMP->SetWorldPos(...);
//   //           pMP->UpdateNormalAndDepth();
//   // BundleAdjustment after a loop (:190-214, nLoopKF != 0): the estimates go to pKF->mTcwGBA / pMP->mPosGBA and
//   //           mnBAGlobalForKF instead of SetPose / SetWorldPos.
//
// LocalBundleAdjustment and BundleAdjustment run the problem in one workgroup: more than MSF_BA_MAX_FREE_CAMS free
// cameras is a failed call.  GlobalBundleAdjustment is Optimizer::GlobalBundleAdjustemnt (:62-69) as
// LoopClosing::RunGlobalBundleAdjustment calls it over the whole map: the same Problem through
// msf_global_bundle_adjust_device (include/msf_global_ba.h), up to MSF_GBA_MAX_FREE_CAMS free cameras, spread over
// the device; where both take a problem they give the same bits.  Header-only and OpenCV-free, like hip_optimizer.h.
// See INTEGRATION.md.
#pragma once

#include <cstdint>
#include <cstring>
#include <vector>

#include "hip_device_block.h"
#include "hip_mirror_types.h"
#include "msf_ba.h"
#include "msf_global_ba.h"

namespace msf {

class BundleAdjuster {
 public:
  struct Edge {
    int32_t camera;   // index into Tcw / fixed
    int32_t point;    // index into points; non-decreasing along the edge list
    Point2f pixel;    // the key point's pixel in that key frame
  };

  struct Problem {
    std::vector<float> Tcw;        // [cameras][16] row-major, in-out: rows 0..2 of a free camera are replaced
    std::vector<uint8_t> fixed;    // [cameras] non-zero: SetFixed(true)
    std::vector<Point3f> points;   // in-out
    std::vector<Edge> edges;
    std::vector<bool> outliers;    // out, [edges]: the edge is in vToErase
    int rounds_run = 0;            // out
  };

  // intrinsics = (fx, fy, cx, cy): one camera.  The calling thread's current HIP device must be the handle's.
  BundleAdjuster(msf_handle* handle, const float intrinsics[4]) : handle_(handle) {
    std::memcpy(intrinsics_, intrinsics, sizeof intrinsics_);
  }

  // :475-527: 5 iterations with the Huber kernel, the classification, 10 without a kernel.  stop: pbStopFlag as the call
  // starts (NULL: none).  false: the problem is left alone.  Either the call failed and msf_last_error(handle) has the
  // text, or the problem was refused without one: here, before any call, for a Tcw that is not 16 floats per camera or
  // for more than MSF_BA_MAX_FREE_CAMS free cameras, or by the kernel (status -1: an edge index out of range, edges not
  // sorted by point).  msf_last_error then holds whatever an earlier call left.
  bool LocalBundleAdjustment(Problem& problem, const int32_t* stop = nullptr) {
    msf_ba_params prm = Params();
    prm.n_rounds = 2;
    prm.iterations[0] = 5, prm.iterations[1] = 10;
    prm.robust[0] = 1, prm.robust[1] = 0;
    return Run(problem, prm, stop);
  }

  // :71-215: one round of nIterations (at most MSF_BA_MAX_ITERATIONS), with the Huber kernel iff bRobust
  bool BundleAdjustment(Problem& problem, int nIterations = 5, bool bRobust = true, const int32_t* stop = nullptr) {
    msf_ba_params prm = Params();
    prm.n_rounds = 1;
    prm.iterations[0] = nIterations;
    prm.robust[0] = bRobust ? 1 : 0;
    return Run(problem, prm, stop);
  }

  // :62-69: BundleAdjustment over the whole map -- every key frame and map point of the caller's Map, key frame 0
  // fixed -- with up to MSF_GBA_MAX_FREE_CAMS free cameras.  The reference's call is (10, false) with
  // pbStopFlag = &mbStopGBA.  stop: the device reads a copy taken as the call starts.  Returns when the problem is
  // finished.  false as for the other two, with MSF_GBA_MAX_FREE_CAMS as the capacity.
  bool GlobalBundleAdjustment(Problem& problem, int nIterations = 10, bool bRobust = false, const int32_t* stop = nullptr) {
    msf_ba_params prm = Params();
    prm.n_rounds = 1;
    prm.iterations[0] = nIterations;
    prm.robust[0] = bRobust ? 1 : 0;
    return Run(problem, prm, stop, true);
  }

 private:
  msf_ba_params Params() const {
    msf_ba_params prm = sized<msf_ba_params>();
    prm.fx = intrinsics_[0], prm.fy = intrinsics_[1], prm.cx = intrinsics_[2], prm.cy = intrinsics_[3];
    prm.huber_delta2 = 5.991, prm.chi2 = 5.991;
    return prm;
  }

  // one block: the descriptor, the problem and the stop word, then status, the poses, the points and the flags
  struct View {
    msf_ba_problem* problem;
    float* Tcw;
    uint8_t* fixed;
    float* points;
    int32_t *edge_cam, *edge_point;
    float* edge_obs;
    int32_t* stop;
    size_t inputs_end;
    msf_ba_result out;
  };

  bool Run(Problem& pb, const msf_ba_params& prm, const int32_t* stop, bool whole_map = false) {
    const size_t nc = pb.fixed.size(), np = pb.points.size(), ne = pb.edges.size();
    if (pb.Tcw.size() != nc * 16) return false;
    DeviceBlock mem;
    View dev, host;
    const auto layout = [&](Carver& c) {
      View v;
      v.problem = c.take<msf_ba_problem>(1);
      v.Tcw = c.take<float>(nc * 12);
      v.fixed = c.take<uint8_t>(nc);
      v.points = c.take<float>(np * 3);
      v.edge_cam = c.take<int32_t>(ne);
      v.edge_point = c.take<int32_t>(ne);
      v.edge_obs = c.take<float>(ne * 2);
      v.stop = c.take<int32_t>(1);
      v.inputs_end = c.off;
      v.out = sized<msf_ba_result>();
      v.out.status = c.take<int32_t>(1);
      v.out.cam_Tcw = c.take<float>(nc * 12);
      v.out.points = c.take<float>(np * 3);
      v.out.outliers = c.take<uint8_t>(ne);
      return v;
    };
    if (!mem.place(layout, &dev, &host)) return false;
    const msf_ba_problem desc = {static_cast<int32_t>(nc), static_cast<int32_t>(np), static_cast<int32_t>(ne), 0, 0, 0};
    *host.problem = desc;
    *host.stop = stop ? *stop : 0;
    int free_cams = 0;
    for (size_t c = 0; c < nc; c++) {
      std::memcpy(host.Tcw + c * 12, &pb.Tcw[c * 16], 48);
      host.fixed[c] = pb.fixed[c];
      free_cams += pb.fixed[c] == 0;
    }
    if (np) std::memcpy(host.points, pb.points.data(), np * sizeof(Point3f));
    for (size_t e = 0; e < ne; e++) {
      host.edge_cam[e] = pb.edges[e].camera, host.edge_point[e] = pb.edges[e].point;
      host.edge_obs[2 * e] = pb.edges[e].pixel.x, host.edge_obs[2 * e + 1] = pb.edges[e].pixel.y;
    }
    if (free_cams > (whole_map ? MSF_GBA_MAX_FREE_CAMS : MSF_BA_MAX_FREE_CAMS)) return false;
    if (!mem.upload()) return false;
    const int32_t max_free = free_cams > 0 ? free_cams : 1;
    const int rc = whole_map
                       ? msf_global_bundle_adjust_device(handle_, desc.n_cams, dev.Tcw, dev.fixed, desc.n_points, dev.points,
                                                         desc.n_edges, dev.edge_cam, dev.edge_point, dev.edge_obs, max_free,
                                                         dev.stop, &prm, &dev.out, nullptr)
                       : msf_bundle_adjust_device(handle_, 1, dev.problem, dev.Tcw, dev.fixed, dev.points, dev.edge_cam,
                                                  dev.edge_point, dev.edge_obs, static_cast<int64_t>(nc),
                                                  static_cast<int64_t>(np), static_cast<int64_t>(ne), max_free, dev.stop,
                                                  &prm, &dev.out, nullptr);
    if (rc != MSF_OK || !mem.download()) return false;
    if (*host.out.status < 0) return false;   // malformed: an edge index out of range or edges not sorted by point
    pb.rounds_run = *host.out.status;
    for (size_t c = 0; c < nc; c++) std::memcpy(&pb.Tcw[c * 16], host.out.cam_Tcw + c * 12, 48);
    if (np) std::memcpy(pb.points.data(), host.out.points, np * sizeof(Point3f));
    pb.outliers.assign(ne, false);
    for (size_t e = 0; e < ne; e++) pb.outliers[e] = host.out.outliers[e] != 0;
    return true;
  }

  msf_handle* handle_;
  float intrinsics_[4];
};

}  // namespace msf
