// csrc/hip_local_mapping.h (msf::NewMapPoints) built with plain g++ against libmsf.so for
// tests/test_local_mapping_mirror_gpu.py: reads 1 + n frames (uint8 [1 + n][480][640]) from argv[1] and 1 + n views
// (msf_view records) from argv[2], stores the frames in slots 0 .. n, runs NewMapPoints of slot 0 against the others and
// writes the created points to argv[3] as raw records {neighbour, match, kp1, kp2, x, y, z}.  Exit 2: no HIP device.
#ifndef __HIP_PLATFORM_AMD__
#define __HIP_PLATFORM_AMD__ 1
#endif
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "hip_local_mapping.h"

int main(int argc, char** argv) {
  if (argc < 5) return 3;
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev == 0) {
    printf("no HIP device\n");
    return 2;
  }
  const int n = atoi(argv[4]), W = 640, H = 480;
  if (n < 1 || n > 8) return 3;
  std::vector<unsigned char> frames((size_t)(1 + n) * W * H);
  std::vector<msf_view> views(1 + n);
  FILE* f = fopen(argv[1], "rb");
  if (!f || fread(frames.data(), 1, frames.size(), f) != frames.size()) return 3;
  fclose(f);
  f = fopen(argv[2], "rb");
  if (!f || fread(views.data(), sizeof(msf_view), views.size(), f) != views.size()) return 3;
  fclose(f);

  msf_config cfg;
  msf_default_config(&cfg, MSF_KIND_ORB);
  cfg.image_width = W;
  cfg.image_height = H;
  cfg.max_batch_pairs = 8;
  msf_handle* h = nullptr;
  if (msf_create(&cfg, &h) != MSF_OK) {
    printf("msf_create: %s\n", msf_last_error(nullptr));
    return 1;
  }
  std::vector<msf::Neighbour> neighbours;
  for (int i = 0; i <= n; i++) {
    const msf_image img = {frames.data() + (size_t)i * W * H, W, H, W};
    if (msf_store_frame(h, i, &img) != MSF_OK) {
      printf("msf_store_frame: %s\n", msf_last_error(h));
      return 1;
    }
    if (i > 0) neighbours.push_back(msf::Neighbour{i, views[i]});
  }
  std::vector<msf::NewMapPoint> created;
  if (!msf::NewMapPoints(h, 0, views[0], neighbours, 1.1, created, 2048)) {
    printf("NewMapPoints: %s\n", msf_last_error(h));
    return 1;
  }
  // no neighbours: true and nothing; a bad slot: false and nothing
  std::vector<msf::NewMapPoint> none(2);
  if (!msf::NewMapPoints(h, 0, views[0], std::vector<msf::Neighbour>(), 1.1, none) || !none.empty()) return 1;
  std::vector<msf::Neighbour> bad(1, msf::Neighbour{99, views[1]});
  if (msf::NewMapPoints(h, 0, views[0], bad, 1.1, none) || !none.empty()) return 1;
  msf_destroy(h);

  FILE* o = fopen(argv[3], "wb");
  if (!o) return 3;
  for (const msf::NewMapPoint& p : created) {
    const int32_t head[6] = {p.neighbour, p.match, p.kp1[0], p.kp1[1], p.kp2[0], p.kp2[1]};
    fwrite(head, 4, 6, o);
    fwrite(&p.x3D, sizeof(msf::Point3f), 1, o);
  }
  fclose(o);
  printf("%zu new points from %d neighbours\n", created.size(), n);
  return 0;
}
