// csrc/hip_pnp_solver.h (msf::PnPsolver) built with plain g++ against libmsf.so for tests/test_pnp_mirror_gpu.py.
// argv[1]: the lists -- int32 count, then per list int32 N, float p3d[N][3], float p2d[N][2]; argv[2]: the log.
// One solver per list (key point indices 2 i + 1 of 2 N + 3 matches, SetRansacParameters as Relocalization sets them),
// their caches filled by one PnPsolver::Prefetch, then iterate(5, ...) round-robin until bNoMore (at most 12 calls each,
// calls after a success included).  The log: one "solver" line each (floor, iterations, the sets) and one "call" line
// per iterate (solver, returned a pose, nInliers, bNoMore, mnIterations, the 16 floats' bits, the true indices).
// Exit 2: no HIP device.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hip_pnp_solver.h"

int main(int argc, char** argv) {
  if (argc < 3) return 3;
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev == 0) {
    printf("no HIP device\n");
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  int32_t count = 0;
  if (!f || fread(&count, 4, 1, f) != 1 || count < 1 || count > 8) return 3;
  msf_config cfg;
  msf_default_config(&cfg, MSF_KIND_ORB);
  cfg.image_width = 640;
  cfg.image_height = 480;
  msf_handle* h = nullptr;
  if (msf_create(&cfg, &h) != MSF_OK) {
    printf("msf_create: %s\n", msf_last_error(nullptr));
    return 1;
  }
  std::vector<msf::PnPsolver*> solvers;
  for (int s = 0; s < count; s++) {
    int32_t n = 0;
    if (fread(&n, 4, 1, f) != 1 || n < 0 || n > 4096) return 3;
    std::vector<msf::Point3f> p3(n);
    std::vector<msf::Point2f> p2(n);
    std::vector<size_t> idx(n);
    if (n && (fread(p3.data(), 12, n, f) != (size_t)n || fread(p2.data(), 8, n, f) != (size_t)n)) return 3;
    for (int i = 0; i < n; i++) idx[i] = 2 * i + 1;
    solvers.push_back(new msf::PnPsolver(h, p3, p2, idx, 2 * n + 3, 520.0f, 515.0f, 318.5f, 242.25f, 99, s));
    solvers.back()->SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991f);
  }
  fclose(f);
  if (!msf::PnPsolver::Prefetch(solvers)) {
    printf("Prefetch: %s\n", msf_last_error(h));
    return 1;
  }
  FILE* o = fopen(argv[2], "w");
  if (!o) return 3;
  std::vector<int> calls(count, 0);
  std::vector<bool> done(count, false);
  std::vector<int> prefetched(count);
  for (int s = 0; s < count; s++) prefetched[s] = solvers[s]->cached();
  for (bool any = true; any;) {
    any = false;
    for (int s = 0; s < count; s++) {
      if (done[s]) continue;
      bool bNoMore = false;
      std::vector<bool> vbInliers;
      int nInliers = -1;
      float Tcw[16];
      std::memset(Tcw, 0, sizeof Tcw);
      const bool ok = solvers[s]->iterate(5, bNoMore, vbInliers, nInliers, Tcw);
      fprintf(o, "call %d %d %d %d %d |", s, ok ? 1 : 0, nInliers, bNoMore ? 1 : 0, solvers[s]->iterations());
      for (int k = 0; k < 16; k++) {
        uint32_t bits;
        std::memcpy(&bits, &Tcw[k], 4);
        fprintf(o, " %u", ok ? bits : 0u);
      }
      fprintf(o, " | %zu", vbInliers.size());
      for (size_t i = 0; i < vbInliers.size(); i++)
        if (vbInliers[i]) fprintf(o, " %zu", i);
      fprintf(o, "\n");
      done[s] = bNoMore || ++calls[s] >= 12;
      any = any || !done[s];
    }
  }
  for (int s = 0; s < count; s++) {
    fprintf(o, "solver %d %d %d %d %d |", s, solvers[s]->minInliers(), solvers[s]->maxIterations(), prefetched[s],
            solvers[s]->cached());
    for (int32_t v : solvers[s]->sets()) fprintf(o, " %d", v);
    fprintf(o, "\n");
    delete solvers[s];
  }
  fclose(o);
  msf_destroy(h);
  printf("%d solvers\n", count);
  return 0;
}
