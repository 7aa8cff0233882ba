// hip_tracking.h -- C++ host mirror of SLAM_PIPELINE::Tracking::SearchLocalPoints (slam_pipeline/src/Tracking.cc:573-633)
// and of the step TrackLocalMap takes behind it (Optimizer::PoseOptimization, :496) above the C ABI
// (include/msf_tracking.h, include/msf_pose.h).
//
// The reference walks mvpLocalKeyFrames: per key frame Frame::isInFrustum on its map points, MatchFrames(current, KF) if
// one is visible, SetMapPoint for every matched key point of the frame that holds no map point; then PoseOptimization
// walks the frame's KeyPointMap.  Here the caller fills a LocalPointSearch with the local map as plain arrays -- the
// point table, the key frames as a CSR over it, the frame's own map -- and
//   Frustum()        stages them through one msf::DeviceBlock and runs msf_frustum_device: visible[] for IncreaseVisible
//                    and n_to_match[] without a match;
//   Search()         is the loop in one call, msf_search_local_points: the claim records, in the order in which the
//                    reference makes its SetMapPoint calls;
//   TrackLocalMap()  chains Search() with MSF_SEARCH_KEEP_ON_DEVICE into msf::Optimizer::PoseOptimizationDevice: the
//                    correspondences never leave the device, only the records, the pose and the flags come back.
// In front of it stands the body of Tracking::TrackWithMotionModel / TrackReferenceKeyFrame (:434-485, :380-424;
// include/msf_frame_tracking.h): the caller fills a FrameTracker with the train frame's map and the point table, and
//   FrameTracker::Track()  is msfx_track_frame: match, carry, PoseOptimization and the cut in one call;
//   TrackFrame()           chains it into TrackLocalMap(): the tracked-frame branch of Tracking::Track in two calls.
// Header-only and OpenCV-free, like hip_local_mapping.h.  What stays with the caller: UpdateLocalKeyFrames, the first
// loop of :576-592 (its result is cur_key / cur_point and the seen flags), IncreaseVisible from `visible`, SetMapPoint from
// `claims`, IncreaseFound.  See INTEGRATION.md.
#pragma once

#include <cstdint>
#include <cstring>
#include <vector>

#include "hip_device_block.h"
#include "hip_mirror_types.h"
#include "hip_optimizer.h"
#include "msf_frame_tracking.h"
#include "msf_tracking.h"

namespace msf {

class LocalPointSearch {
 public:
  // ---- in: the local map of the tracked frame (include/msf_tracking.h: msf_local_map) ----
  std::vector<msf_map_point> points;   // GetWorldPos(), GetNormal(), GetDistanceInvariance(), MSF_POINT_BAD | MSF_POINT_SEEN
  std::vector<int32_t> slots;          // [n_kf]: where msf_store_frame put each local key frame
  std::vector<int32_t> kf_start;       // [n_kf + 1], or empty for no key frame
  std::vector<int32_t> kf_key, kf_point;     // per entry: the pixel key y * cols + x (increasing inside a key frame), the point
  std::vector<int32_t> cur_key, cur_point;   // the frame's own map, keys increasing
  msf_frustum_params params = sized<msf_frustum_params>();   // mRcw, mtcw, intrinsics, GetCameraCenter(), mnMinX .. mnMaxY, 0.5

  // ---- out ----
  std::vector<uint8_t> status, visible;      // [n_points]: the frustum code, and status == 0 (IncreaseVisible)
  std::vector<int32_t> owner_kf;             // [n_points]
  std::vector<int32_t> n_to_match;           // [n_kf]: nToMatch of each key frame
  std::vector<int32_t> num_matches;          // [n_kf]: the list's length, -1 for a key frame that was not matched
  std::vector<msf_local_claim> claims;       // SetMapPoint(key, point), in the reference's order
  std::vector<int32_t> n_claimed;            // [n_kf]
  int32_t n_corr = 0;                        // the frame's own map + the claims: what PoseOptimization gets

  int32_t n_kf() const { return kf_start.empty() ? 0 : static_cast<int32_t>(kf_start.size()) - 1; }

  // Steps 1-2 alone on the map staged in a block allocated here: status, visible, owner_kf, n_to_match.  The calling thread's current HIP device
  // must be the handle's.  false: a failed call (msf_last_error(handle) has the text) or a malformed map.
  bool Frustum(msf_handle* handle) {
    if (!handle || !Consistent()) return false;
    const size_t np = points.size(), nk = static_cast<size_t>(n_kf()), ne = kf_key.size(), nc = cur_key.size();
    // one block: the point table, the CSR and the frame's map, then the results
    struct View {
      msf_map_point* points;
      int32_t *kf_start, *kf_key, *kf_point, *cur_key, *cur_point;
      size_t inputs_end;
      msf_frustum_result out;
    };
    DeviceBlock block;
    View dev, host;
    const auto layout = [&](Carver& c) {
      View v;
      v.points = c.take<msf_map_point>(np);
      v.kf_start = c.take<int32_t>(nk + 1);
      v.kf_key = c.take<int32_t>(ne);
      v.kf_point = c.take<int32_t>(ne);
      v.cur_key = c.take<int32_t>(nc);
      v.cur_point = c.take<int32_t>(nc);
      v.inputs_end = c.off;
      v.out = sized<msf_frustum_result>();
      v.out.status_word = c.take<int32_t>(1);
      v.out.n_to_match = c.take<int32_t>(nk);
      v.out.status = c.take<uint8_t>(np);
      v.out.visible = c.take<uint8_t>(np);
      v.out.owner_kf = c.take<int32_t>(np);
      return v;
    };
    if (!block.place(layout, &dev, &host)) return false;
    Copy(host.points, points);
    Copy(host.kf_start, kf_start);
    Copy(host.kf_key, kf_key);
    Copy(host.kf_point, kf_point);
    Copy(host.cur_key, cur_key);
    Copy(host.cur_point, cur_point);
    const msf_local_map map = Map(dev.points, dev.kf_start, dev.kf_key, dev.kf_point, dev.cur_key, dev.cur_point);
    if (!block.upload() || msf_frustum_device(handle, &map, &params, &dev.out, nullptr) != MSF_OK || !block.download() ||
        host.out.status_word[0] != 0)
      return false;
    status.assign(host.out.status, host.out.status + np);
    visible.assign(host.out.visible, host.out.visible + np);
    owner_kf.assign(host.out.owner_kf, host.out.owner_kf + np);
    n_to_match.assign(host.out.n_to_match, host.out.n_to_match + nk);
    return true;
  }

  // The loop in one call: the stored frame query_slot against `slots`; at most max_batch_pairs key frames; `cap`:
  // matches kept per key frame.  Fills visible, n_to_match, num_matches, claims, n_claimed, n_corr.  `kept`: null, or
  // where the correspondences stay on the device (MSF_SEARCH_KEEP_ON_DEVICE).  A matched key frame without a valid list
  // (MSF_ERR_CAPACITY) contributes nothing and the others are kept, as a failed MatchFrames would leave an empty list.
  // false: the call failed (msf_last_error(handle) has the text) and the results are empty.
  bool Search(msf_handle* handle, int32_t query_slot, int32_t cap = 4096, msf_device_corr* kept = nullptr) {
    claims.clear();
    n_corr = 0;
    if (!handle || cap < 1 || !Consistent() || slots.size() != static_cast<size_t>(n_kf())) return false;
    const size_t np = points.size(), nk = static_cast<size_t>(n_kf());
    status.assign(np, 0);
    visible.assign(np, 0);
    owner_kf.assign(np, 0);
    n_to_match.assign(nk, 0);
    num_matches.assign(nk, 0);
    n_claimed.assign(nk, 0);
    std::vector<msf_local_claim> records(nk * static_cast<size_t>(cap) + 1);
    int32_t words[2] = {0, 0}, n_claims = 0;
    msf_frustum_result fr = sized<msf_frustum_result>();
    fr.status_word = &words[0], fr.n_to_match = n_to_match.data();
    fr.status = status.data(), fr.visible = visible.data(), fr.owner_kf = owner_kf.data();
    msf_claim_result cl = sized<msf_claim_result>();
    cl.status_word = &words[1], cl.n_claims = &n_claims, cl.n_claimed = n_claimed.data();
    cl.claims = records.data(), cl.n_corr = &n_corr;
    if (kept) *kept = sized<msf_device_corr>();
    const msf_local_map map = Map(points.data(), kf_start.data(), kf_key.data(), kf_point.data(), cur_key.data(), cur_point.data());
    const int rc = msf_search_local_points(handle, query_slot, slots.data(), &map, &params,
                                           kept ? MSF_SEARCH_KEEP_ON_DEVICE : 0u, num_matches.data(), nullptr, cap, &fr, &cl, kept);
    if (rc != MSF_OK && rc != MSF_ERR_CAPACITY) {
      n_corr = 0;
      return false;
    }
    claims.assign(records.begin(), records.begin() + (n_claims > 0 ? n_claims : 0));
    return true;
  }

 private:
  bool Consistent() const {
    return kf_key.size() == kf_point.size() && cur_key.size() == cur_point.size() && (!kf_start.empty() || kf_key.empty());
  }

  msf_local_map Map(const msf_map_point* p, const int32_t* start, const int32_t* key, const int32_t* point,
                    const int32_t* ckey, const int32_t* cpoint) const {
    msf_local_map m = sized<msf_local_map>();
    m.n_points = static_cast<int32_t>(points.size()), m.n_kf = n_kf();
    m.n_entries = static_cast<int32_t>(kf_key.size()), m.n_cur = static_cast<int32_t>(cur_key.size());
    m.points = p, m.kf_start = start, m.kf_key = key, m.kf_point = point, m.cur_key = ckey, m.cur_point = cpoint;
    return m;
  }

  template <class T>
  static void Copy(T* dst, const std::vector<T>& src) {
    if (!src.empty()) std::memcpy(dst, src.data(), src.size() * sizeof(T));
  }
};

// Tracking::TrackLocalMap from SearchLocalPoints to the optimised pose (Tracking.cc:489-496): search.Search() with the
// correspondences kept on the device, then Optimizer::PoseOptimization on them where they are.  Tcw in: mCurrentFrame's
// mTcw (row-major [16]), out: the optimised pose; outliers[i]: the flag of correspondence i -- i < cur_key.size() is the
// frame's own entry i, the others are search.claims in order.  The calling thread's current HIP device must be the
// handle's.  -> nInitialCorrespondences - nBad; -1: a call failed (Tcw and outliers are left alone).
inline int TrackLocalMap(msf_handle* handle, int32_t query_slot, LocalPointSearch& search, float Tcw[16],
                         std::vector<bool>& outliers, int32_t cap = 4096, float chi2 = 5.991f) {
  msf_device_corr kept;
  if (!search.Search(handle, query_slot, cap, &kept) || search.n_corr < 0) return -1;
  if (kept.corr_cap < 1) {   // neither an entry of the frame nor a key frame: nothing to optimise (Optimizer.cc:253)
    outliers.clear();
    return 0;
  }
  const float intrinsics[4] = {search.params.view.fx, search.params.view.fy, search.params.view.cx, search.params.view.cy};
  return Optimizer::PoseOptimizationDevice(handle, kept.d_corr_p3d, kept.d_corr_p2d, kept.corr_cap, kept.d_n_corr,
                                           intrinsics, Tcw, outliers, chi2);
}

// The body of Tracking::TrackWithMotionModel (train = the last frame, cur_* empty after Clear()) and of
// TrackReferenceKeyFrame (train = the reference key frame; cur_* = what the frame holds when it runs as the fallback).
class FrameTracker {
 public:
  // ---- in (include/msf_frame_tracking.h: msfx_frame_map, msfx_track_params) ----
  std::vector<msf_map_point> points;         // the point table that goes on to LocalPointSearch; only pos is read here
  std::vector<uint8_t> observed;             // [n_points]: Observations() > 0; empty: every point is observed
  std::vector<int32_t> ref_key, ref_point;   // the train frame's mKeyPointMap, keys y * cols + x increasing
  std::vector<int32_t> cur_key, cur_point;   // the current frame's own map at entry, keys increasing
  float intrinsics[4] = {0, 0, 0, 0};        // fx, fy, cx, cy
  float chi2 = 5.991f;
  int32_t min_matches = 15, min_map_matches = 10;   // mMinLocalMatchCount, and the 10 of :422 / :483

  // ---- out ----
  int32_t track_status = -1;                 // 0 tracked, 1 too few matches, 2 too few map matches; negative: no result
  int32_t num_matches = 0, n_good = -1, n_matches_map = 0;
  std::vector<msfx_frame_point> map;         // the frame's map after the carry, key order; flags bit 0: removed by the cut
  std::vector<int32_t> kept_key, kept_point; // the frame's map at return: LocalPointSearch::cur_key / cur_point
  std::vector<msfx_removed_point> removed;   // SetMapPoint(key, nullptr); mnLastFrameSeen is still due to these points

  // The stored frame query_slot against the stored frame train_slot.  Tcw in: the entry pose (row-major [16]; mVelocity *
  // mLastFrame.mTcw, or the last frame's), out: the optimised pose when the call gave a result (track_status >= 0).
  // `kept`: null, or where the results stay on the device (MSFX_TRACK_KEEP_ON_DEVICE).  true: the frame is tracked
  // (track_status == 0).  false with track_status < 0: a failed call (msf_last_error(handle) has the text), a malformed
  // map, no room or no valid list.
  bool Track(msf_handle* handle, int32_t query_slot, int32_t train_slot, float Tcw[16], int32_t cap = 4096,
             msfx_device_track* kept = nullptr) {
    track_status = -1, num_matches = 0, n_good = -1, n_matches_map = 0;
    map.clear(), kept_key.clear(), kept_point.clear(), removed.clear();
    if (!handle || cap < 1 || ref_key.size() != ref_point.size() || cur_key.size() != cur_point.size() ||
        (!observed.empty() && observed.size() != points.size()))
      return false;
    const size_t room = cur_key.size() + static_cast<size_t>(cap);
    msfx_frame_map m = sized<msfx_frame_map>();
    m.n_points = static_cast<int32_t>(points.size()), m.n_ref = static_cast<int32_t>(ref_key.size());
    m.n_cur = static_cast<int32_t>(cur_key.size());
    m.points = points.data(), m.observed = observed.empty() ? nullptr : observed.data();
    m.ref_key = ref_key.data(), m.ref_point = ref_point.data(), m.cur_key = cur_key.data(), m.cur_point = cur_point.data();
    msfx_track_params prm = sized<msfx_track_params>();
    prm.pose = sized<msf_pose_params>();
    prm.pose.fx = intrinsics[0], prm.pose.fy = intrinsics[1], prm.pose.cx = intrinsics[2], prm.pose.cy = intrinsics[3];
    prm.pose.chi2 = chi2;
    std::memcpy(prm.Tcw0, Tcw, sizeof prm.Tcw0);
    prm.min_matches = min_matches, prm.min_map_matches = min_map_matches;
    std::vector<msfx_frame_point> recs(room + 1);
    std::vector<int32_t> keys(room + 1), pts(room + 1);
    std::vector<msfx_removed_point> gone(room + 1);
    int32_t counts[3] = {0, 0, 0};
    float pose[12];
    msfx_track_result out = sized<msfx_track_result>();
    out.track_status = &track_status, out.n_map = &counts[0], out.map = recs.data();
    out.Tcw = pose, out.n_good = &n_good, out.n_kept = &counts[1], out.kept_key = keys.data(), out.kept_point = pts.data();
    out.n_removed = &counts[2], out.removed = gone.data(), out.n_matches_map = &n_matches_map;
    if (kept) *kept = sized<msfx_device_track>();
    const int rc = msfx_track_frame(handle, query_slot, train_slot, &m, &prm, kept ? MSFX_TRACK_KEEP_ON_DEVICE : 0u,
                                    &num_matches, nullptr, cap, &out, nullptr, kept);
    if (rc != MSF_OK || track_status < 0) {   // MSF_ERR_CAPACITY included: no valid list, as a failed MatchFrames
      if (track_status >= 0) track_status = -1;
      return false;
    }
    map.assign(recs.begin(), recs.begin() + counts[0]);
    kept_key.assign(keys.begin(), keys.begin() + counts[1]);
    kept_point.assign(pts.begin(), pts.begin() + counts[1]);
    removed.assign(gone.begin(), gone.begin() + counts[2]);
    std::memcpy(Tcw, pose, sizeof pose);
    return track_status == 0;
  }
};

// The tracked-frame branch of Tracking::Track (Tracking.cc:120-140): TrackWithMotionModel or TrackReferenceKeyFrame,
// then TrackLocalMap.  tracker.Track() against train_slot; on success the frame's map at return becomes search's
// cur_key / cur_point, the points of kept and removed alike get MSF_POINT_SEEN in search.points (the reference's
// mnLastFrameSeen covers both, Tracking.cc:576-592 and :416), the current frame's view in search.params takes the new
// pose -- mRcw, mtcw and mOw = -mRcw' mtcw, f32 products summed left to right as the solve headers do for a cv::Mat
// product -- and TrackLocalMap() runs on search.slots.  search.points must be the table tracker.points indexes.
// -> TrackLocalMap's count; -1: a call failed; -2: the frame was not tracked (tracker.track_status says why).
inline int TrackFrame(msf_handle* handle, int32_t query_slot, int32_t train_slot, FrameTracker& tracker,
                      LocalPointSearch& search, float Tcw[16], std::vector<bool>& outliers, int32_t cap = 4096,
                      float chi2 = 5.991f) {
  if (search.points.size() != tracker.points.size()) return -1;
  tracker.chi2 = chi2;
  if (!tracker.Track(handle, query_slot, train_slot, Tcw, cap)) return tracker.track_status < 0 ? -1 : -2;
  search.cur_key = tracker.kept_key;
  search.cur_point = tracker.kept_point;
  for (int32_t p : tracker.kept_point) search.points[static_cast<size_t>(p)].flags |= MSF_POINT_SEEN;
  for (const msfx_removed_point& r : tracker.removed) search.points[static_cast<size_t>(r.point)].flags |= MSF_POINT_SEEN;
  msf_view& v = search.params.view;
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) v.Rcw[3 * r + c] = Tcw[4 * r + c];
    v.tcw[r] = Tcw[4 * r + 3];
  }
  for (int c = 0; c < 3; c++) {
    float sum = 0.0f;
    for (int r = 0; r < 3; r++) sum += v.Rcw[3 * r + c] * v.tcw[r];
    search.params.Ow[c] = -sum;
  }
  return TrackLocalMap(handle, query_slot, search, Tcw, outliers, cap, chi2);
}

}  // namespace msf
