// msf::BundleAdjuster::GlobalBundleAdjustment (csrc/hip_bundle_adjustment.h) built with plain g++ against libmsf.so
// for tests/test_gba_mirror_gpu.py.  argv[1]: the problem in the format of tests/cpp/test_ba_mirror.cpp; argv[2]: the
// log.  The problem goes through GlobalBundleAdjustment(10, false) ("global") and through it with the stop word set
// ("stopped"): the rounds run, the bits of every Tcw and point afterwards, the indices of the flagged edges.  Exit 2: no
// HIP device.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hip_bundle_adjustment.h"

static void log_line(FILE* o, const char* kind, const msf::BundleAdjuster::Problem& p) {
  fprintf(o, "%s %d |", kind, p.rounds_run);
  for (float v : p.Tcw) {
    uint32_t bits;
    std::memcpy(&bits, &v, 4);
    fprintf(o, " %u", bits);
  }
  fprintf(o, " |");
  for (const msf::Point3f& q : p.points) {
    uint32_t bits[3];
    std::memcpy(bits, &q, 12);
    fprintf(o, " %u %u %u", bits[0], bits[1], bits[2]);
  }
  fprintf(o, " | %zu", p.outliers.size());
  for (size_t i = 0; i < p.outliers.size(); i++)
    if (p.outliers[i]) fprintf(o, " %zu", i);
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
  int32_t n[3] = {0, 0, 0};
  if (!f || fread(n, 4, 3, f) != 3 || n[0] < 0 || n[0] > 4096 || n[1] < 0 || n[1] > 65536 || n[2] < 0 || n[2] > 1000000) return 3;
  msf::BundleAdjuster::Problem in;
  in.Tcw.resize((size_t)n[0] * 16), in.fixed.resize(n[0]), in.points.resize(n[1]), in.edges.resize(n[2]);
  std::vector<int32_t> ec(n[2]), ep(n[2]);
  std::vector<float> obs((size_t)n[2] * 2);
  bool ok = (!n[0] || (fread(in.Tcw.data(), 64, n[0], f) == (size_t)n[0] && fread(in.fixed.data(), 1, n[0], f) == (size_t)n[0]));
  ok = ok && (!n[1] || fread(in.points.data(), 12, n[1], f) == (size_t)n[1]);
  ok = ok && (!n[2] || (fread(ec.data(), 4, n[2], f) == (size_t)n[2] && fread(ep.data(), 4, n[2], f) == (size_t)n[2] &&
                         fread(obs.data(), 8, n[2], f) == (size_t)n[2]));
  if (!ok) return 3;
  fclose(f);
  for (int e = 0; e < n[2]; e++) in.edges[e] = {ec[e], ep[e], {obs[2 * e], obs[2 * e + 1]}};
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
  const float K[4] = {500.0f, 500.0f, 320.0f, 240.0f};
  msf::BundleAdjuster ba(h, K);
  msf::BundleAdjuster::Problem global = in, stopped = in;
  global.outliers.assign(3, true);   // stale content that the call must replace
  const int32_t stop = 1;
  if (!ba.GlobalBundleAdjustment(global) || !ba.GlobalBundleAdjustment(stopped, 10, false, &stop)) {
    printf("BundleAdjuster: %s\n", msf_last_error(h));
    return 1;
  }
  log_line(o, "global", global);
  log_line(o, "stopped", stopped);
  // a malformed problem is a failed call that leaves the problem alone
  msf::BundleAdjuster::Problem bad = in;
  if (!bad.edges.empty()) {
    bad.edges[bad.edges.size() / 2].camera = n[0];
    if (ba.GlobalBundleAdjustment(bad) || bad.Tcw != in.Tcw || !bad.outliers.empty()) {
      printf("a malformed problem was not refused\n");
      return 1;
    }
  }
  fclose(o);
  msf_destroy(h);
  printf("%d cameras %d points %d edges\n", n[0], n[1], n[2]);
  return 0;
}
