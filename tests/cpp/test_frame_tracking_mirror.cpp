// csrc/hip_tracking.h (msf::FrameTracker, msf::TrackFrame) built with plain g++ against libmsf.so for
// tests/test_frame_tracking_mirror_gpu.py.  argv[1]: 1 + n frames (uint8 [1 + n][480][640]), frame 1 being the train
// frame and 1 .. n the local key frames; argv[2]: int32 {n_points, n_ref, n_cur, n_kf, n_entries, has_observed}, then
// points, observed (if any), ref_key, ref_point, cur_key, cur_point, kf_start [n_kf + 1], kf_key, kf_point, the
// msf_frustum_params (intrinsics and bounds; the view's pose is set by TrackFrame) and the entry pose float [16];
// argv[3]: the output -- int32 {track_status, num_matches, n_good, n_matches_map, n_map, n_kept, n_removed,
// final n_good, n_corr, n_claims}, the records, kept_key, kept_point, removed, the pose of Track() [16], the claim
// records, the pose of TrackFrame() [16] and one flag byte per correspondence.  Exit 2: no HIP device.
#ifndef __HIP_PLATFORM_AMD__
#define __HIP_PLATFORM_AMD__ 1
#endif
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "hip_tracking.h"

template <class T>
static bool read(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

template <class T>
static void write(FILE* f, const std::vector<T>& v) {
  if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f);
}

int main(int argc, char** argv) {
  if (argc < 4) return 3;
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev == 0) {
    printf("no HIP device\n");
    return 2;
  }
  const int W = 640, H = 480;
  FILE* f = fopen(argv[2], "rb");
  int32_t head[6];
  if (!f || fread(head, 4, 6, f) != 6) return 3;
  const int n = head[3];
  if (n < 1 || n > 8) return 3;
  msf::FrameTracker tracker;
  msf::LocalPointSearch search;
  float Tcw0[16];
  if (!read(f, tracker.points, head[0]) || !read(f, tracker.observed, head[5] ? head[0] : 0) ||
      !read(f, tracker.ref_key, head[1]) || !read(f, tracker.ref_point, head[1]) || !read(f, tracker.cur_key, head[2]) ||
      !read(f, tracker.cur_point, head[2]) || !read(f, search.kf_start, (size_t)n + 1) || !read(f, search.kf_key, head[4]) ||
      !read(f, search.kf_point, head[4]) || fread(&search.params, sizeof search.params, 1, f) != 1 || fread(Tcw0, 4, 16, f) != 16)
    return 3;
  fclose(f);
  search.points = tracker.points;
  const msf_view& v = search.params.view;
  tracker.intrinsics[0] = v.fx, tracker.intrinsics[1] = v.fy, tracker.intrinsics[2] = v.cx, tracker.intrinsics[3] = v.cy;
  std::vector<unsigned char> frames((size_t)(1 + n) * W * H);
  f = fopen(argv[1], "rb");
  if (!f || fread(frames.data(), 1, frames.size(), f) != frames.size()) return 3;
  fclose(f);

  msf_config cfg;
  msf_default_config(&cfg, MSF_KIND_ORB);
  cfg.threshold = 0.8f;
  cfg.image_width = W;
  cfg.image_height = H;
  cfg.max_batch_pairs = 8;
  msf_handle* h = nullptr;
  if (msf_create(&cfg, &h) != MSF_OK) {
    printf("msf_create: %s\n", msf_last_error(nullptr));
    return 1;
  }
  for (int i = 0; i <= n; i++) {
    const msf_image img = {frames.data() + (size_t)i * W * H, W, H, W};
    if (msf_store_frame(h, i, &img) != MSF_OK) {
      printf("msf_store_frame: %s\n", msf_last_error(h));
      return 1;
    }
    if (i > 0) search.slots.push_back(i);
  }
  // the body alone
  float Tcw[16];
  for (int k = 0; k < 16; k++) Tcw[k] = Tcw0[k];
  const bool tracked = tracker.Track(h, 0, 1, Tcw, 2048);
  if (tracker.track_status < 0) {
    printf("Track: %s\n", msf_last_error(h));
    return 1;
  }
  const msf::FrameTracker first = tracker;
  // and the two calls of the tracked-frame branch
  float Tfinal[16];
  for (int k = 0; k < 16; k++) Tfinal[k] = Tcw0[k];
  std::vector<bool> outliers;
  const int n_good = msf::TrackFrame(h, 0, 1, tracker, search, Tfinal, outliers, 2048);
  if (n_good == -1 || (n_good == -2) == tracked) {
    printf("TrackFrame: %d, %s\n", n_good, msf_last_error(h));
    return 1;
  }
  if (tracker.map.size() != first.map.size() || tracker.kept_key != first.kept_key || tracker.n_good != first.n_good) {
    printf("Track() twice disagrees\n");
    return 1;
  }
  // a bad slot: false and no result; a malformed map: the same
  msf::FrameTracker bad = first;
  float T2[16];
  for (int k = 0; k < 16; k++) T2[k] = Tcw0[k];
  if (bad.Track(h, 0, 99, T2) || bad.track_status >= 0 || !bad.map.empty() || T2[3] != Tcw0[3]) return 1;
  bad = first;
  bad.ref_point[0] = head[0];
  if (bad.Track(h, 0, 1, T2) || bad.track_status >= 0) return 1;
  msf_destroy(h);

  FILE* o = fopen(argv[3], "wb");
  if (!o) return 3;
  const int32_t out_head[10] = {first.track_status, first.num_matches, first.n_good, first.n_matches_map,
                                (int32_t)first.map.size(), (int32_t)first.kept_key.size(), (int32_t)first.removed.size(),
                                n_good, n_good >= 0 ? search.n_corr : 0, (int32_t)search.claims.size()};
  fwrite(out_head, 4, 10, o);
  write(o, first.map);
  write(o, first.kept_key);
  write(o, first.kept_point);
  write(o, first.removed);
  fwrite(Tcw, 4, 16, o);
  write(o, search.claims);
  fwrite(Tfinal, 4, 16, o);
  for (bool b : outliers) fputc(b ? 1 : 0, o);
  fclose(o);
  printf("track_status %d, %d matches, %zu records, %zu kept, n_good %d; then %zu claims, n_good %d\n", first.track_status,
         first.num_matches, first.map.size(), first.kept_key.size(), first.n_good, search.claims.size(), n_good);
  return 0;
}
