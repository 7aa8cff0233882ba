// csrc/hip_initializer.h (msf::Initialize) built with plain g++ against libmsf.so for
// tests/test_initializer_mirror_gpu.py: reads a match list (int32 [n][4]) from argv[1], runs Initialize with the K of the
// test scenes and writes ok, R21, t21, vP3D and vbTriangulated to argv[2] as raw bytes.  Exit 2: no HIP device.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "hip_initializer.h"

int main(int argc, char** argv) {
  if (argc < 5) return 3;
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev == 0) {
    printf("no HIP device\n");
    return 2;
  }
  std::vector<msf_match> matches;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  msf_match m;
  while (fread(&m, sizeof m, 1, f) == 1) matches.push_back(m);
  fclose(f);
  const int iterations = atoi(argv[3]);
  const unsigned long long seed = strtoull(argv[4], nullptr, 10);

  msf_config cfg;
  msf_default_config(&cfg, MSF_KIND_ORB);
  cfg.image_width = 640;
  cfg.image_height = 480;
  msf_handle* h = nullptr;
  if (msf_create(&cfg, &h) != MSF_OK) {
    printf("msf_create: %s\n", msf_last_error(nullptr));
    return 1;
  }
  const float K[9] = {500.f, 0.f, 320.f, 0.f, 500.f, 240.f, 0.f, 0.f, 1.f};
  float R21[9], t21[3];
  std::vector<msf::Point3f> vP3D;
  std::vector<bool> vbTriangulated;
  const bool ok = msf::Initialize(h, matches, K, 1.0f, iterations, seed, 50, 1.0f, R21, t21, vP3D, vbTriangulated);
  // too few matches: false, nothing touched
  std::vector<msf_match> few(matches.begin(), matches.begin() + (matches.size() < 7 ? matches.size() : 7));
  std::vector<msf::Point3f> p2(3);
  std::vector<bool> b2(3, true);
  float R2[9], t2[3];
  if (msf::Initialize(h, few, K, 1.0f, iterations, seed, 50, 1.0f, R2, t2, p2, b2) || p2.size() != 3 || b2.size() != 3 || R2[0] != 0.f) {
    printf("a list of %zu matches must give false and leave the vectors alone\n", few.size());
    return 1;
  }
  msf_destroy(h);

  FILE* o = fopen(argv[2], "wb");
  if (!o) return 3;
  const int32_t okv = ok ? 1 : 0, np = (int32_t)vP3D.size();
  fwrite(&okv, 4, 1, o);
  fwrite(&np, 4, 1, o);
  fwrite(R21, 4, 9, o);
  fwrite(t21, 4, 3, o);
  for (int i = 0; i < np; i++) {
    fwrite(&vP3D[i], sizeof(msf::Point3f), 1, o);
  }
  for (int i = 0; i < np; i++) {
    const unsigned char b = vbTriangulated[i] ? 1 : 0;
    fwrite(&b, 1, 1, o);
  }
  fclose(o);
  printf("ok %d, %d points\n", okv, np);
  return 0;
}
