// Host build of csrc/triangulate_solve.h (the arithmetic of triangulate_kernels.hip) for
// tests/test_new_points_host.py: g++ -ffp-contract=off, loaded with ctypes, checked against a float64 reference.
#include "triangulate_solve.h"

using namespace msf::triangulate;

static_assert(sizeof(View) == 64, "msf_view layout");

extern "C" {

// One list, sequentially, as k_new_points leaves it: status [n], points [n][3], hom [n][4], cos [n], packed [n][4]
// (match index, then the bits of x, y, z) in match order.  Returns n_new.
int new_points_host_run(int n, const int32_t* matches, const View* v1, const View* v2, double max_cos, double chi2,
                        uint8_t* status, float* points, float* hom, double* cos, int32_t* packed) {
  int n_new = 0;
  for (int i = 0; i < n; i++) {
    const Match m{matches[4 * i], matches[4 * i + 1], matches[4 * i + 2], matches[4 * i + 3]};
    const int s = new_point(m, *v1, *v2, max_cos, chi2, points + 3 * i, hom + 4 * i, cos + i);
    status[i] = (uint8_t)s;
    if (s == kNewPoint) {
      union { float f; int32_t i; } b;
      packed[4 * n_new] = i;
      for (int k = 0; k < 3; k++) {
        b.f = points[3 * i + k];
        packed[4 * n_new + 1 + k] = b.i;
      }
      n_new++;
    }
  }
  return n_new;
}
}
