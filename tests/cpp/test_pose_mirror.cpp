// csrc/hip_optimizer.h (msf::Optimizer) built with plain g++ against libmsf.so for tests/test_pose_mirror_gpu.py.
// argv[1]: the lists -- int32 count, then per list int32 N, float Tcw[16], float p3d[N][3], float p2d[N][2]; argv[2]:
// the log.  Every list goes through PoseOptimization alone ("single" lines) and all of them through one
// PoseOptimizationBatch ("batch" lines): list, the return, the 16 floats' bits of Tcw afterwards, the size of the flag
// vector and the indices that are true.  Exit 2: no HIP device.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hip_optimizer.h"

struct List {
  std::vector<msf::Point3f> p3;
  std::vector<msf::Point2f> p2;
  float Tcw[16];
};

static void log_line(FILE* o, const char* kind, int s, int good, const float* Tcw, const std::vector<bool>& flags) {
  fprintf(o, "%s %d %d |", kind, s, good);
  for (int k = 0; k < 16; k++) {
    uint32_t bits;
    std::memcpy(&bits, &Tcw[k], 4);
    fprintf(o, " %u", bits);
  }
  fprintf(o, " | %zu", flags.size());
  for (size_t i = 0; i < flags.size(); i++)
    if (flags[i]) fprintf(o, " %zu", i);
  fprintf(o, "\n");
}

int main(int argc, char** argv) {
  if (argc < 3) return 3;
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev == 0) {
    printf("no HIP device\n");
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  int32_t count = 0;
  if (!f || fread(&count, 4, 1, f) != 1 || count < 1 || count > 16) return 3;
  std::vector<List> lists(count);
  for (List& l : lists) {
    int32_t n = 0;
    if (fread(&n, 4, 1, f) != 1 || n < 0 || n > 4096 || fread(l.Tcw, 4, 16, f) != 16) return 3;
    l.p3.resize(n), l.p2.resize(n);
    if (n && (fread(l.p3.data(), 12, n, f) != (size_t)n || fread(l.p2.data(), 8, n, f) != (size_t)n)) return 3;
  }
  fclose(f);
  msf_config cfg;
  msf_default_config(&cfg, MSF_KIND_ORB);
  cfg.image_width = 640;
  cfg.image_height = 480;
  msf_handle* h = nullptr;
  if (msf_create(&cfg, &h) != MSF_OK) {
    printf("msf_create: %s\n", msf_last_error(nullptr));
    return 1;
  }
  FILE* o = fopen(argv[2], "w");
  if (!o) return 3;
  const float K[4] = {520.0f, 515.0f, 318.5f, 242.25f};
  for (int s = 0; s < count; s++) {
    float Tcw[16];
    std::memcpy(Tcw, lists[s].Tcw, sizeof Tcw);
    std::vector<bool> flags(3, true);   // stale content that the call must replace
    const int good = msf::Optimizer::PoseOptimization(h, lists[s].p3, lists[s].p2, K, Tcw, flags);
    if (good < 0) {
      printf("PoseOptimization: %s\n", msf_last_error(h));
      return 1;
    }
    log_line(o, "single", s, good, Tcw, flags);
  }
  std::vector<std::vector<bool>> flags(count, std::vector<bool>(5, true));
  std::vector<List> work = lists;
  std::vector<msf::Optimizer::Candidate> cands;
  for (int s = 0; s < count; s++) cands.push_back({&work[s].p3, &work[s].p2, work[s].Tcw, &flags[s], -7});
  if (!msf::Optimizer::PoseOptimizationBatch(h, cands, K)) {
    printf("PoseOptimizationBatch: %s\n", msf_last_error(h));
    return 1;
  }
  for (int s = 0; s < count; s++) log_line(o, "batch", s, cands[s].n_good, work[s].Tcw, flags[s]);
  fclose(o);
  msf_destroy(h);
  printf("%d lists\n", count);
  return 0;
}
