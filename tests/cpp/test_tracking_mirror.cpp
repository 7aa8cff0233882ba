// csrc/hip_tracking.h (msf::LocalPointSearch, msf::TrackLocalMap) built with plain g++ against libmsf.so for
// tests/test_tracking_mirror_gpu.py.  argv[1]: 1 + n frames (uint8 [1 + n][480][640]); argv[2]: the local map -- int32
// {n_points, n_kf, n_entries, n_cur}, then points, kf_start [n_kf + 1], kf_key, kf_point, cur_key, cur_point, the
// msf_frustum_params and the entry pose float [16]; argv[3]: the output -- int32 {n_claims, n_corr, n_good, n_points,
// n_kf}, the claim records, num_matches, n_to_match of Search(), n_to_match / status / visible / owner_kf of Frustum(),
// the optimised pose [16] and one flag byte per correspondence.  Exit 2: no HIP device.
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
  int32_t head[4];
  if (!f || fread(head, 4, 4, f) != 4) return 3;
  const int n = head[1];
  if (n < 1 || n > 8) return 3;
  msf::LocalPointSearch search;
  float Tcw[16];
  if (!read(f, search.points, head[0]) || !read(f, search.kf_start, (size_t)n + 1) || !read(f, search.kf_key, head[2]) ||
      !read(f, search.kf_point, head[2]) || !read(f, search.cur_key, head[3]) || !read(f, search.cur_point, head[3]) ||
      fread(&search.params, sizeof search.params, 1, f) != 1 || fread(Tcw, 4, 16, f) != 16)
    return 3;
  fclose(f);
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
  // the frustum test alone, on the staged map
  if (!search.Frustum(h)) {
    printf("Frustum: %s\n", msf_last_error(h));
    return 1;
  }
  const std::vector<int32_t> f_to_match = search.n_to_match, f_owner = search.owner_kf;
  const std::vector<uint8_t> f_status = search.status, f_visible = search.visible;
  // the loop and the pose behind it
  std::vector<bool> outliers;
  const int n_good = msf::TrackLocalMap(h, 0, search, Tcw, outliers, 2048);
  if (n_good < 0) {
    printf("TrackLocalMap: %s\n", msf_last_error(h));
    return 1;
  }
  if (search.status != f_status || search.visible != f_visible || search.owner_kf != f_owner || search.n_to_match != f_to_match) {
    printf("Frustum() and Search() disagree\n");
    return 1;
  }
  // a bad slot: false, -1 and nothing; a malformed map: Frustum() says no
  msf::LocalPointSearch bad = search;
  bad.slots[0] = 99;
  float T2[16];
  std::vector<bool> o2(3, true);
  if (bad.Search(h, 0) || !bad.claims.empty() || msf::TrackLocalMap(h, 0, bad, T2, o2) != -1 || o2.size() != 3) return 1;
  bad = search;
  bad.kf_point[0] = head[0];
  if (bad.Frustum(h)) return 1;
  msf_destroy(h);

  FILE* o = fopen(argv[3], "wb");
  if (!o) return 3;
  const int32_t out_head[5] = {(int32_t)search.claims.size(), search.n_corr, n_good, head[0], n};
  fwrite(out_head, 4, 5, o);
  write(o, search.claims);
  write(o, search.num_matches);
  write(o, search.n_to_match);
  write(o, f_to_match);
  write(o, f_status);
  write(o, f_visible);
  write(o, f_owner);
  fwrite(Tcw, 4, 16, o);
  for (bool b : outliers) fputc(b ? 1 : 0, o);
  fclose(o);
  printf("%zu claims, %d correspondences, n_good %d\n", search.claims.size(), search.n_corr, n_good);
  return 0;
}
